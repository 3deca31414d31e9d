"""Every stage on the context's own stream, behind a busy device: the table of tests/stream_common.py executed on the three kinds of
stream (null: torch's current stream in a pytest process, the HIP null stream; own: the non-blocking stream vrt_ctx_create makes;
side: a torch side stream).  Per (case, kind): buffers made and poisoned, one torch.cuda.synchronize(), the set-up steps, the
stall, the sequence without a synchronise by the caller, one vrt_ctx_synchronize, then every output against the oracle or the
numpy definitions, bit for bit.  Expected values are computed once per case and shared by the three kinds."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import launch_shapes_common as lsc
import raygen_reference as rays_ref
import render_rays_common as rr
import reproject_cam_common as rcc
import reproject_common as rc
import reproject_reference as rp_ref
import scene_reference as R
import stream_common as sc
import upsample_common as uc
from denoise_shard_common import owned_rows
from helpers import camera_push, compare_planes, metallic_palette
from ray_query_common import oracle_records, planes_differ

pytestmark = pytest.mark.gpu

P = C.c_void_p
SPEC = {"color8": (np.uint8, (4,)), "depth": (np.float32, ()), "motion": (np.float32, (2,)), "mask8": (np.uint8, ()),
        "position": (np.float32, (4,)), "normal8": (np.int8, (4,)), "color_f": (np.float32, (3,)), "hit_id": (np.uint8, ()),
        "hit_voxel": (np.int16, (3,)), "hit_mask": (np.uint8, ()), "steps_primary": (np.int32, ()), "steps_total": (np.int32, ()),
        "rays_total": (np.int32, ())}
GB = ("color8", "depth", "motion", "mask8", "position", "normal8")
DIAG = ("hit_voxel", "steps_primary", "steps_total")          # host.DIAGNOSTIC_MARCH_PLANES: rendered in a launch of their own
PLANE_SETS = {"gbuffer": GB, "launch": GB + ("hit_id",), "debug": GB + ("color_f", "hit_id", "hit_voxel", "hit_mask", "steps_primary", "steps_total", "rays_total"),
              "rays": rr.ALL_PLANES}
TORCH = {np.uint8: torch.uint8, np.int8: torch.int8, np.int16: torch.int16, np.int32: torch.int32, np.float32: torch.float32}
_expected = {}          # (case id, what) -> value, shared by the kinds and never changed
_redone = {}            # case id -> the null run's counts
_rehearsed = set()      # cases that have run on null in this process: their kernels are loaded, their helper streams' first use is over


def _args(a, *more):
    """A step's arguments (but for the name of its output) as a key: everything an expected value depends on."""
    return repr(sorted((k, v) for k, v in a.items() if k != "out")) + repr(more)


def _once(key, make):
    if key not in _expected:
        _expected[key] = make()
    return _expected[key]


def _settings(vrt, which, res):
    st = vrt.VoxelRenderSettings.primary_only(res) if which == "primary_only" else vrt.VoxelRenderSettings(targetResolution=tuple(res))
    st.fsrSetttings.enable = False
    if which == "default_ao2":
        st.occlusionSettings.numSamples = 2
    if which == "split":
        st.traceSettings.splitKernels = True
    assert which in ("primary_only", "default", "default_ao2", "split") and tuple(st.renderResolution()) == tuple(res)
    return st.to_c()


class Run:
    """One (case, kind): the engine, the buffers, the numpy side of the scenes, and the launch / verify closures of the steps."""

    def __init__(self, vrt, oracle, case, kind):
        self.vrt, self.oracle, self.case, self.kind = vrt, oracle, case, kind
        self.lib, self.cap = vrt.lib(), vrt._capi
        self.engine = vrt.Engine(0, use_torch_stream=kind != "own")
        self.dev = self.engine.torch_device
        self.scenes, self.bufs, self.keep, self.verifies = {}, {}, [], []
        self.vol, self.sky, self.noise, self.pal = {}, {}, {}, metallic_palette(vrt)
        self.stall_buf = None
        self.rays, self.images, self.sums, self.frame_exp = {}, {}, {}, {}
        self.group = "E-tags" if case.id.startswith("E-tags") else case.id        # (the two tags cases render the same frames)

    # ---- buffers ----------------------------------------------------------------------------------------------------------------
    def buf(self, name, shape, dtype):
        """A device tensor of the poison byte, kept under `name`."""
        n = int(np.prod(shape, dtype=np.int64)) * np.dtype(dtype).itemsize
        t = torch.full((n,), sc.POISON, dtype=torch.uint8, device=self.dev).view(TORCH[dtype]).reshape(tuple(shape))
        self.bufs[name] = t
        return t

    def upload(self, name, array):
        t = torch.from_numpy(np.ascontiguousarray(array)).to(self.dev)
        self.bufs[name] = t
        return t

    def planes(self, out, res, names, n=1):
        """n frames of the named planes: ({plane: tensor (n, H, W, ...)}, Frame * n)"""
        W, H = res
        ts = {p: self.buf(f"{out}.{p}", (n, H, W) + SPEC[p][1], SPEC[p][0]) for p in names}
        frames = (self.cap.Frame * n)()
        for f in range(n):
            for p, t in ts.items():
                setattr(frames[f], p, t[f].data_ptr())
        return ts, frames

    def host(self, ts, f=0):
        return {p: t[f].cpu().numpy() for p, t in ts.items()}

    def check(self, rc):
        self.cap.check(rc)

    # ---- the stall ----------------------------------------------------------------------------------------------------------------
    def prepare_stall(self):
        if self.kind == "own":
            p = P()
            self.check(self.lib.vrt_device_alloc(self.engine.ctx, sc.STALL_BYTES, C.byref(p)))
            self.stall_buf = p
        else:
            self.stall_buf = torch.zeros(sc.STALL_BYTES // 4, dtype=torch.float32, device=self.dev)

    def stall(self):
        """A few milliseconds of work on the context's stream: what is enqueued next waits behind it."""
        for k in range(sc.STALL_PASSES):
            if self.kind == "own":
                self.check(self.lib.vrt_memset(self.engine.ctx, self.stall_buf, k, sc.STALL_BYTES))
            else:
                self.stall_buf.add_(1.0)

    def close(self):
        for s in self.scenes.values():
            s.destroy()
        if self.kind == "own" and self.stall_buf is not None:
            self.lib.vrt_device_free(self.engine.ctx, self.stall_buf)
        self.stall_buf = None
        self.bufs.clear()
        self.engine.destroy()

    # ---- the numpy side of a frame --------------------------------------------------------------------------------------------
    def oracle_scene(self, scene):
        return self.oracle.OracleScene(np.array(self.vol[scene]), self.pal, sky=self.sky[scene], noise=self.noise[scene])

    def oracle_frames(self, a, scene, stc, pushes, names):
        """a: the step's arguments.  The key holds them all, the output's name too: the scene changes along a sequence, and the
        outputs' names are unique within a case (tests/test_stream_cases_cpu.py)."""
        osn = self.oracle_scene(scene)           # (the scene as it is at this step of the walk)
        pr = self.oracle.params_from(stc)
        key = (a["out"], _args(a))
        return lambda: _once((self.group, key), lambda: [self.oracle.render(osn, p, pr, planes=list(names), nthreads=8) for p in pushes])

    def push_of(self, a, scene):
        dims = self.vol[scene].shape[::-1]
        if "seq" in a:
            which, k = a["seq"]
            if which == "reproject":
                return rc.pushes_of(self.vrt, self.oracle, a["res"][0], a["res"][1], frames=2)[k]
            return uc.pushes_of(self.vrt, self.oracle, sc.UPSAMPLE_PAIR, frames=2)[k]
        if "tags_pose" in a:
            return camera_push(self.vrt, dims, a["res"], **lsc.TAGS_POSES[a["tags_pose"]])
        return camera_push(self.vrt, dims, a["res"], **a["pose"])

    # ---- scenes -------------------------------------------------------------------------------------------------------------------
    def h_vrt_scene_from_dense(self, a):
        vol = sc.volume(self.vrt, a["volume"])
        self.vol[a["scene"]], self.sky[a["scene"]], self.noise[a["scene"]] = vol, None, None

        def launch():
            self.scenes[a["scene"]] = self.vrt.VoxelScene.from_dense(self.engine, vol, self.pal)
        return launch, None

    def h_vrt_scene_from_bricks(self, a):
        vol = sc.volume(self.vrt, a["volume"])
        grid, pool = self.vrt.synthetic.bricks_from_dense(np.array(vol))
        self.vol[a["scene"]], self.sky[a["scene"]], self.noise[a["scene"]] = vol, None, None
        self.bricks0 = int(pool.shape[0])

        def launch():
            self.scenes[a["scene"]] = self.vrt.VoxelScene.from_bricks(self.engine, grid, pool, self.pal)
        return launch, None

    def h_vrt_scene_set_sky(self, a):
        img = sc.sky(self.vrt, a["sky"])
        self.sky[a["scene"]] = img
        return (lambda: self.scenes[a["scene"]].set_sky(img)), None

    def h_vrt_scene_set_blue_noise(self, a):
        img = sc.noise(self.vrt, a["noise"])
        self.noise[a["scene"]] = img
        return (lambda: self.scenes[a["scene"]].set_blue_noise(img)), None

    def h_vrt_scene_edit_box(self, a):
        ids = sc.box_ids(a["ids"])
        self.vol[a["scene"]] = sc.apply_box(self.vol[a["scene"]], a["lo"], ids)
        return (lambda: self.scenes[a["scene"]].edit(a["lo"], ids)), None

    def h_vrt_scene_fill_box(self, a):
        self.vol[a["scene"]] = sc.apply_box(self.vol[a["scene"]], a["lo"], a["id"], a["size"])
        return (lambda: self.scenes[a["scene"]].fill(a["lo"], a["size"], a["id"])), None

    def h_vrt_scene_reserve_bricks(self, a):
        self.capacity = self.bricks0 + a["extra"]
        return (lambda: self.scenes[a["scene"]].reserve_bricks(self.capacity)), None

    def h_vrt_scene_download(self, a):
        vol, got = np.array(self.vol[a["scene"]]), {}

        def launch():
            got["vox"], got["pal"] = self.scenes[a["scene"]].download()

        def verify():
            assert (got["vox"] == vol).all(), "vrt_scene_download: the voxels differ"
            assert (got["pal"].view(np.uint32) == np.asarray(self.pal, np.float32).view(np.uint32)).all(), "vrt_scene_download: the palette differs"
        return launch, verify

    def h_vrt_debug_scene_state(self, a):
        vol, got, what = np.array(self.vol[a["scene"]]), {}, f"case {self.case.id} on {self.kind}"

        def launch():
            for n in a["what"]:
                got[n] = self.scenes[a["scene"]].debug_state(getattr(self.cap, "STATE_" + n))

        def verify():
            D, H, W = vol.shape
            if "VOX" in got:
                assert (got["VOX"] == vol.reshape(-1)).all(), (what, "VOX")
                exp = _once((self.case.id, "df"), lambda: R.dense_df_bytes(vol, True))
                assert got["DF"].size == exp.size, (what, "DF size")
                assert R.diff_df(got["DF"], exp, (W, H, D), what) is None, R.diff_df(got["DF"], exp, (W, H, D), what)
                for k, (name, ref) in enumerate(zip(("OCC1", "OCC2", "OCC3"), R.pyramid(vol))):
                    msg = R.diff_words(got[name], ref, name, R.level_dims((W, H, D), k + 1), what)
                    assert msg is None, msg
                msg = R.diff_cells(got["CELLS"], R.cells(vol), what)
                assert msg is None, msg
            else:
                nb = (W // 8, H // 8, D // 8)
                ent, pool, fine = got["BENTRY"], got["BPOOL"], got["BFINE"]
                expect = _once((self.case.id, "entries"), lambda: R.brick_entries(R.brick_occupancy(vol), True))
                msg = R.diff_entries(ent, expect, nb, self.capacity, what)
                assert msg is None, msg
                assert pool.shape == (self.capacity, 512) and fine.shape == (self.capacity, 8, 512), (what, pool.shape, fine.shape)
                msg = R.diff_brick_bytes(ent, pool, fine, vol, nb, what)
                assert msg is None, msg
                msg = R.diff_cells(got["CELLS"], R.brick_cells(vol), what)
                assert msg is None, msg
        return launch, verify

    def h_vrt_ctx_set_option(self, a):
        def launch():
            self.engine.set_option(a["option"], a["value"])
            assert self.engine.option(a["option"]) == a["value"]
        return launch, None

    # ---- the geometry stage ----------------------------------------------------------------------------------------------------
    def h_vrt_render_geometry(self, a):
        names = PLANE_SETS[a["planes"]]
        stc, push = _settings(self.vrt, a["settings"], a["res"]), self.push_of(a, a["scene"])
        ts, frames = self.planes(a["out"], a["res"], names)
        shard = self.cap.Shard(*a["shard"]) if a.get("shard") else None
        calls = [frames[0]]
        if a["planes"] == "debug":               # as GeometryBuffer.to_c_split: the product march, then the diagnostic one
            product, diag = self.cap.Frame(), self.cap.Frame()
            for p in names:
                setattr(diag if p in DIAG else product, p, getattr(frames[0], p))
            calls = [product, diag]
        self.keep += [stc, push, frames, shard, calls]
        exp = self.frame_exp[a["out"]] = self.oracle_frames(a, a["scene"], stc, [push], names)

        def launch():
            for fr in calls:
                self.check(self.lib.vrt_render_geometry(self.engine.ctx, self.scenes[a["scene"]].handle, C.byref(push), C.byref(stc), C.byref(fr),
                                                        C.byref(shard) if shard is not None else None))

        def verify():
            self.same_frame(a["out"], self.host(ts), exp()[0], names, a["res"], a.get("shard"))
        return launch, verify

    def same_frame(self, what, got, exp, names, res, shard=None):
        """Own rows equal the oracle's; with a shard, every other row still holds the poison."""
        own = np.ones(res[1], bool)
        if shard:
            own[:] = False
            own[owned_rows(res[1], *shard)] = True
            assert own.any() and not own.all()
            for p in names:
                assert (got[p][~own].view(np.uint8) == sc.POISON).all(), (self.case.id, self.kind, what, p, "a row of another rank was written")
        bad = compare_planes({p: got[p][own] for p in names}, {p: exp[p][own] for p in names}, names)
        assert not bad, (self.case.id, self.kind, what, bad)

    def _batch(self, a, fn, shards=None):
        names = PLANE_SETS["launch"]
        dims = self.vol[a["scene"]].shape[::-1]
        if "tags_poses" in a:
            lo, hi = a["tags_poses"]
            pushes = [camera_push(self.vrt, dims, a["res"], **p) for p in lsc.poses(lsc.TAGS_POOL, dims)][lo:hi]
        else:
            lo, hi = a["poses"]
            pushes = [camera_push(self.vrt, dims, a["res"], **p) for p in lsc.poses(hi, dims)][lo:hi]
        n = len(pushes)
        stc, arr = _settings(self.vrt, a["settings"], a["res"]), (self.cap.Push * n)(*pushes)
        ts, frames = self.planes(a["out"], a["res"], names, n)
        cs = (self.cap.Shard * n)(*[self.cap.Shard(*s) for s in shards]) if shards else None
        self.keep += [stc, arr, frames, cs]
        exp = self.oracle_frames(a, a["scene"], stc, pushes, names)

        def launch():
            self.check(fn(self.engine.ctx, self.scenes[a["scene"]].handle, n, arr, C.byref(stc), frames, cs))

        def verify():
            e = exp()
            for f in range(n):
                self.same_frame(f"{a['out']}[{f}]", self.host(ts, f), e[f], names, a["res"], shards[f] if shards else None)
        return launch, verify

    def h_vrt_render_geometry_batch(self, a):
        return self._batch(a, self.lib.vrt_render_geometry_batch)

    def h_vrt_render_geometry_slots(self, a):
        lo, hi = a["poses"]
        return self._batch(a, self.lib.vrt_render_geometry_slots, [(f % a["ranks"], a["ranks"], a["strip_rows"]) for f in range(hi - lo)])

    # ---- rays -----------------------------------------------------------------------------------------------------------------------
    def controller(self, a):
        W, H, D = sc.DIMS[a["dims"]]
        return self.vrt.CameraController(position=(W / 2.0 + 0.37, H / 2.0 + 0.21, -0.8 * D))          # helpers.camera_push's

    def h_vrt_camera_rays(self, a):
        W, H = a["res"]
        cap = self.cap
        if a["model"] == "panorama":
            cam, exp = self.vrt.RayCamera.panorama(a["at"]).to_c((W, H)), lambda: rays_ref.camera_rays(rays_ref.PANORAMA, W, H, pos=a["at"])
        elif a["model"] == "perspective":
            ctl, jitter = self.controller(a), a["pose"]["jitter"]
            cam = self.vrt.RayCamera.perspective(ctl, 90.0).to_c((W, H), jitter)
            assert cam.tan_half == 1.0
            exp = lambda: rays_ref.camera_rays(rays_ref.PERSPECTIVE, W, H, pos=ctl.position, cam_dir=ctl.direction, right=ctl.right, up=ctl.up,
                                               jitter=jitter, tan_half=1.0)
        else:
            cam = cap.RayCamera()
            cam.model = cap.CAMERA_ORTHOGRAPHIC
            o = rr.ORTHO
            cam.basis.cam_pos[:] = list(o["pos"]) + [1.0]
            cam.basis.cam_dir[:] = list(o["cam_dir"]) + [0.0]
            cam.basis.cam_right[:] = list(o["right"]) + [0.0]
            cam.basis.cam_up[:] = list(o["up"]) + [0.0]
            cam.basis.screen_size[:] = [W, H]
            cam.tan_half, cam.half_width = 1.0, o["half_width"]
            exp = lambda: rr.ortho_rays(W, H)
        o, d = self.buf(a["out"] + ".o", (W * H, 3), np.float32), self.buf(a["out"] + ".d", (W * H, 3), np.float32)
        self.keep.append(cam)
        self.rays[a["out"]] = (o, d, lambda: _once(("rays", _args(a)), exp), _args(a))

        def launch():
            self.check(self.lib.vrt_camera_rays(self.engine.ctx, C.byref(cam), W, H, P(o.data_ptr()), P(d.data_ptr())))

        def verify():
            eo, ed = self.rays[a["out"]][2]()
            go, gd = o.cpu().numpy(), d.cpu().numpy()
            assert (go.view(np.uint32) == eo.view(np.uint32)).all(), (self.case.id, self.kind, a["out"], "origins")
            assert (gd.view(np.uint32) == ed.view(np.uint32)).all(), (self.case.id, self.kind, a["out"], "directions")
        return launch, verify

    def records(self, scene, rays, max_steps):
        """The oracle's records of the DEFINITION's rays (the device's rays are held to them by the vrt_camera_rays step)."""
        osn, exp, made_by = self.oracle_scene(scene), self.rays[rays][2], self.rays[rays][3]
        return lambda: _once((self.case.id, "records", made_by, max_steps), lambda: oracle_records(self.oracle, osn, *exp(), max_steps)[0])

    def hits(self, out, n):
        ts = {"material": self.buf(out + ".material", (n,), np.uint8), "pos": self.buf(out + ".pos", (n, 3), np.float32),
              "voxel": self.buf(out + ".voxel", (n, 3), np.int32), "normal": self.buf(out + ".normal", (n, 3), np.int8)}
        h = self.cap.RayHits(**{k: P(t.data_ptr()) for k, t in ts.items()})
        self.keep.append(h)
        return ts, h

    def h_vrt_trace_rays(self, a):
        o, d = self.rays[a["rays"]][:2]
        n = int(o.shape[0])
        ts, h = self.hits(a["out"], n)
        exp = self.records(a["scene"], a["rays"], a["max_steps"])

        def launch():
            self.check(self.lib.vrt_trace_rays(self.engine.ctx, self.scenes[a["scene"]].handle, n, P(o.data_ptr()), P(d.data_ptr()), a["max_steps"], C.byref(h)))

        def verify():
            e = exp()
            assert (e["material"] != 0).any() and (e["material"] == 0).any()
            bad = planes_differ({k: t.cpu().numpy() for k, t in ts.items()}, e)
            assert bad.size == 0, (self.case.id, self.kind, a["out"], bad[:8].tolist(), bad.size)
        return launch, verify

    def h_vrt_occluded_rays(self, a):
        o, d = self.rays[a["rays"]][:2]
        n = int(o.shape[0])
        occ = self.buf(a["out"], (n,), np.uint8)
        exp = self.records(a["scene"], a["rays"], a["max_steps"])

        def launch():
            self.check(self.lib.vrt_occluded_rays(self.engine.ctx, self.scenes[a["scene"]].handle, n, P(o.data_ptr()), P(d.data_ptr()), a["max_steps"], P(occ.data_ptr())))

        def verify():
            e = (exp()["material"] != 0).astype(np.uint8)
            assert e.any() and not e.all()
            bad = np.flatnonzero(occ.cpu().numpy() != e)
            assert bad.size == 0, (self.case.id, self.kind, a["out"], bad[:8].tolist(), bad.size)
        return launch, verify

    def perspective_push(self, a):
        return self.vrt.make_push(self.controller(a), sc.DIMS[a["dims"]], a["res"], a["pose"]["frame"], a["pose"]["jitter"])

    def h_vrt_render_rays(self, a):
        W, H = a["res"]
        o, d = self.rays[a["rays"]][:2]
        names = PLANE_SETS["rays"]
        ts, frames = self.planes(a["out"], a["res"], names)
        stc = _settings(self.vrt, a["settings"], a["res"])
        src = next(st.args for st in self.case.steps if st.name == "vrt_camera_rays" and st.args["out"] == a["rays"])
        push = self.perspective_push(src)        # tan_half = 1: the rays are the built-in camera's of this push
        assert src["model"] == "perspective" and push.frame == a["frame"]
        self.keep += [stc, frames]
        exp = self.oracle_frames(a, a["scene"], stc, [push], names)

        def launch():
            self.check(self.lib.vrt_render_rays(self.engine.ctx, self.scenes[a["scene"]].handle, W, H, P(o.data_ptr()), P(d.data_ptr()), a["frame"],
                                                C.byref(stc), C.byref(frames[0])))

        def verify():
            e = exp()[0]
            assert (e["hit_id"] != 0).any() and (e["hit_id"] == 0).any()
            self.same_frame(a["out"], self.host(ts), e, names, a["res"])
        return launch, verify

    def h_vrt_pick_pixels(self, a):
        W, H = a["res"]
        ys, xs = np.mgrid[0:H, 0:W]
        xy = self.upload(a["out"] + ".xy", np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.int32))
        ts, h = self.hits(a["out"], W * H)
        push = self.perspective_push(a)
        self.keep.append(push)
        rays = next(st.args["out"] for st in self.case.steps if st.name == "vrt_camera_rays" and st.args["model"] == "perspective")
        exp = self.records(a["scene"], rays, a["max_steps"])

        def launch():
            self.check(self.lib.vrt_pick_pixels(self.engine.ctx, self.scenes[a["scene"]].handle, C.byref(push), a["max_steps"], W * H, P(xy.data_ptr()), C.byref(h)))

        def verify():
            bad = planes_differ({k: t.cpu().numpy() for k, t in ts.items()}, exp())
            assert bad.size == 0, (self.case.id, self.kind, a["out"], bad[:8].tolist(), bad.size)
        return launch, verify

    def h_vrt_debug_sky_texels(self, a):
        """The kernel's own comparison (spec texel, fast texel, sure) over the definition's panorama directions, on the sky in force."""
        W, H = a["dirs"][1]
        d = self.upload(a["out"] + ".d", rays_ref.camera_rays(rays_ref.PANORAMA, W, H, pos=(0.0, 0.0, 0.0))[1])
        out = self.buf(a["out"], (W * H, 4), np.int32)
        sky = self.sky[a["scene"]]

        def launch():
            self.check(self.lib.vrt_debug_sky_texels(self.engine.ctx, self.scenes[a["scene"]].handle, P(d.data_ptr()), W * H, P(out.data_ptr())))

        def verify():
            g = out.cpu().numpy()
            sure = g[:, 2] != 0
            assert sure.mean() > 0.1 and (g[sure, 0] == g[sure, 1]).all(), (self.case.id, self.kind, a["out"])
            assert len(np.unique(g[:, 0])) == sky.shape[0] * sky.shape[1], "a panorama of 64 x 32 directions sees every texel of the 7 x 5 sky"
        return launch, verify

    def h_vrt_debug_spec(self, a):
        """One primitive of the numeric spec over n pairs of spec_common's edge set, against the oracle's vo_spec_batch."""
        import spec_common as sp
        kind, n = a["pairs"]
        assert kind == "edges"
        e = sp.edge_set()
        y, x = np.resize(e, n), np.resize(e[::-1][5:], n)
        yd, xd = self.upload(a["out"] + ".y", y.view(np.int32)), self.upload(a["out"] + ".x", x.view(np.int32))
        out = self.buf(a["out"], (n + 64,), np.int32)
        exp = _once((self.group, a["out"], _args(a)), lambda: self.oracle.spec_batch(a["fn"], y, x, nthreads=8))

        def launch():
            self.check(self.lib.vrt_debug_spec(self.engine.ctx, a["fn"], P(yd.data_ptr()), P(xd.data_ptr()), None, n, P(out.data_ptr())))

        def verify():
            g = out.cpu().numpy().view(np.uint32)
            assert (g[n:] == np.uint32(sc.POISON * 0x01010101)).all(), (self.case.id, self.kind, a["out"], "wrote past its n elements")
            sp.hold(g[:n], exp, a["fn"], (y, x), f"case {self.case.id} on {self.kind}: vrt_debug_spec")
        return launch, verify

    # ---- strip and halo copies (the numpy row maps of voxel-raytracing_amd/distributed.py) ---------------------------------------
    GUARD = 2

    def copy_step(self, a, fn, unpack, halo, batch):
        """One of the eight copies.  Packed buffers have the rows of their own shard plus GUARD rows nobody may write; an unpack goes
        into a poisoned frame, of which only the mapped rows may change.  Expected bytes: pack_np / unpack_np."""
        D = self.vrt.distributed
        (W, H), bpp, S, hl = a["res"], a["bpp"], a["strip_rows"], a["halo"]
        n, rb = a.get("n", 1), W * bpp
        shards = [tuple(a["shard"])] * n if "shard" in a else lsc.copy_shards(n)
        maps = [(lsc.halo_map(H, r, N, S, hl, a["direction"], D) if halo else lsc.own_row_map(H, r, N, S, D)) for r, N in shards]
        assert len({len(m) for m in maps}) == 1
        rows = len(maps[0])
        fulls = _once(("copy images", n, H, rb), lambda: np.random.default_rng(100 * n + bpp).integers(0, 256, (n, H, rb), dtype=np.uint8))
        if a["src"] in ("full", "fulls") and a["src"] not in self.bufs:
            self.upload(a["src"], fulls)
        src = self.bufs[a["src"]]
        dst = self.buf(a["out"], (n, H, rb) if unpack else (n, rows + self.GUARD, rb), np.uint8)
        cs = (self.cap.Shard * n)(*[self.cap.Shard(r, N, S) for r, N in shards])
        ptrs = lambda t: (P * n)(*[t[i].data_ptr() for i in range(n)])
        sp, dp = ptrs(src), ptrs(dst)
        self.keep += [cs, sp, dp]
        tail = (hl, a["direction"]) if halo else ()
        one = "shard" in a and fn.__name__ == "vrt_pack_rows_batch"          # the one batch form that takes one shard for all

        def launch():
            if batch:
                self.check(fn(self.engine.ctx, n, sp, dp, W, H, bpp, C.byref(cs[0]) if one else cs, *tail))
            else:
                self.check(fn(self.engine.ctx, P(src[0].data_ptr()), P(dst[0].data_ptr()), W, H, bpp, C.byref(cs[0]), *tail))

        def verify():
            got = dst.cpu().numpy()
            for i, m in enumerate(maps):
                ok = m >= 0
                packed = D.pack_np(fulls[i], m)
                if unpack:
                    want = np.full((H, rb), sc.POISON, np.uint8)
                    D.unpack_np(packed, want, m)
                    assert (got[i] == want).all(), (self.case.id, self.kind, a["out"], i, "only mapped rows may change")
                else:
                    assert (got[i, :rows][ok] == packed[ok]).all(), (self.case.id, self.kind, a["out"], i, "packed rows differ")
                    assert np.isin(got[i, :rows][~ok], (0, sc.POISON)).all(), (self.case.id, self.kind, a["out"], i, "a padding row holds image bytes")
                    assert (got[i, rows:] == sc.POISON).all(), (self.case.id, self.kind, a["out"], i, "written past the end of the packed buffer")
        return launch, verify

    def h_vrt_pack_rows(self, a):
        return self.copy_step(a, self.lib.vrt_pack_rows, False, False, False)

    def h_vrt_unpack_rows(self, a):
        return self.copy_step(a, self.lib.vrt_unpack_rows, True, False, False)

    def h_vrt_pack_halo(self, a):
        return self.copy_step(a, self.lib.vrt_pack_halo, False, True, False)

    def h_vrt_unpack_halo(self, a):
        return self.copy_step(a, self.lib.vrt_unpack_halo, True, True, False)

    def h_vrt_pack_rows_batch(self, a):
        return self.copy_step(a, self.lib.vrt_pack_rows_batch, False, False, True)

    def h_vrt_unpack_rows_batch(self, a):
        return self.copy_step(a, self.lib.vrt_unpack_rows_batch, True, False, True)

    def h_vrt_pack_halo_batch(self, a):
        return self.copy_step(a, self.lib.vrt_pack_halo_batch, False, True, True)

    def h_vrt_unpack_halo_batch(self, a):
        return self.copy_step(a, self.lib.vrt_unpack_halo_batch, True, True, True)

    # ---- the post chain ---------------------------------------------------------------------------------------------------------
    def gbuffer(self, name):
        """(device planes, lambda: the oracle's planes) of a frame a vrt_render_geometry step of this case wrote."""
        return {p: self.bufs[f"{name}.{p}"][0] for p in GB}, lambda: self.frame_exp[name]()[0]

    def image(self, name):
        """(device tensor holder, lambda: expected) of an RGBA8 image an earlier step made."""
        return self.images[name]

    def h_vrt_denoise(self, a):
        W, H = a["res"]
        g, gexp = self.gbuffer(a["src"])
        t0, t1 = self.buf(a["out"] + ".t0", (H, W, 4), np.uint8), self.buf(a["out"] + ".t1", (H, W, 4), np.uint8)
        ds = self.cap.DenoiserSettings(a["iterations"], 20.4, 1e-2, 1e-1, 2.0, a["mode"])
        res, holder = P(), {}
        self.keep.append(ds)

        def exp():
            e = gexp()
            return _once((self.case.id, a["out"]), lambda: self.oracle.denoise(e["color8"], e["normal8"], e["position"], iterations=a["iterations"], mode=a["mode"]))
        self.images[a["out"]] = (holder, exp)

        def launch():
            self.check(self.lib.vrt_denoise(self.engine.ctx, W, H, C.byref(ds), g["color8"].data_ptr(), g["normal8"].data_ptr(), g["position"].data_ptr(),
                                            t0.data_ptr(), t1.data_ptr(), None, C.byref(res)))
            holder["t"] = t0 if res.value == t0.data_ptr() else t1
            assert res.value in (t0.data_ptr(), t1.data_ptr())

        def verify():
            bad = np.flatnonzero((holder["t"].cpu().numpy() != exp()).any((1, 2)))
            assert bad.size == 0, (self.case.id, self.kind, a["out"], "rows", bad[:8].tolist())
        return launch, verify

    def h_vrt_accumulate(self, a):
        W, H = a["res"]
        holder, exp = self.image(a["src"])
        if a["reset"]:
            self.buf(a["acc"], (H, W, 4), np.int32)
            self.sums[a["acc"]] = []
        acc = self.bufs[a["acc"]]
        self.sums[a["acc"]].append(exp)

        def launch():
            self.check(self.lib.vrt_accumulate(self.engine.ctx, holder["t"].data_ptr(), acc.data_ptr(), W, H, a["reset"]))
        return launch, None

    def h_vrt_resolve(self, a):
        W, H = a["res"]
        acc, out, parts, n = self.bufs[a["acc"]], self.buf(a["out"], (H, W, 4), np.uint8), self.sums[a["acc"]], a["frames"]
        assert len(parts) == n

        def exp():
            s = sum(p().astype(np.int64) for p in parts)
            return ((2 * s + n) // (2 * n)).astype(np.uint8)
        self.images[a["out"]] = ({"t": out}, exp)

        def launch():
            self.check(self.lib.vrt_resolve(self.engine.ctx, acc.data_ptr(), out.data_ptr(), W, H, n))

        def verify():
            s = sum(p().astype(np.int64) for p in parts)
            assert (acc.cpu().numpy().astype(np.int64) == s).all(), (self.case.id, self.kind, a["acc"])
            assert (out.cpu().numpy() == exp()).all(), (self.case.id, self.kind, a["out"])
        return launch, verify

    def h_vrt_blit(self, a):
        (W, H), (TW, TH) = a["res"], a["target"]
        holder, exp = self.image(a["src"])
        out = self.buf(a["out"], (TH, TW, 4), np.uint8)

        def launch():
            self.check(self.lib.vrt_blit(self.engine.ctx, holder["t"].data_ptr(), W, H, out.data_ptr(), TW, TH))

        def verify():
            assert (out.cpu().numpy() == self.oracle.blit(exp(), TW, TH)).all(), (self.case.id, self.kind, a["out"])
        return launch, verify

    def temporal(self, a, family, rows, cols, call, definition):
        """A step of one of the three temporal passes: frame 0 starts the sequence into history pair 0, frame 1 reads it and writes
        pair 1; every frame has its own resolved image and motion plane."""
        f = a["frame"]
        if f == 0:
            for k in range(2):
                self.buf(f"{family}.h{k}.color16", (rows, cols, 4), np.int16)
                self.buf(f"{family}.h{k}.surface", (rows, cols, 4), np.int32)
        pair = lambda k: self.cap.History(self.bufs[f"{family}.h{k}.color16"].data_ptr(), self.bufs[f"{family}.h{k}.surface"].data_ptr())
        hin, hout = (pair(f - 1) if f else None), pair(f)
        resolved, motion = self.buf(a["out"] + ".resolved8", (rows, cols, 4), np.uint8), self.buf(a["out"] + ".motion", (rows, cols, 2), np.float32)
        self.keep += [hin, hout]

        def launch():
            self.check(call(hin, hout, resolved, motion))

        def verify():
            e = _once((self.case.id, family), definition)[f]
            got = {"color16": self.bufs[f"{family}.h{f}.color16"].cpu().numpy().view(np.uint16), "surface": self.bufs[f"{family}.h{f}.surface"].cpu().numpy().view(np.uint32),
                   "resolved8": resolved.cpu().numpy(), "motion": motion.cpu().numpy()}
            assert rp_ref.same(got, e) == [], (self.case.id, self.kind, a["out"], rp_ref.same(got, e))
        return launch, verify

    def sequence_frames(self, prefix):
        """lambda: [(color8, position, normal8)] by the oracle of the frames the steps g0, g1 / u0, u1 rendered"""
        return lambda: [(e["color8"], e["position"], e["normal8"]) for e in (self.frame_exp[f"{prefix}{k}"]()[0] for k in range(2))]

    def h_vrt_reproject(self, a):
        W, H = a["res"]
        pushes = rc.pushes_of(self.vrt, self.oracle, W, H, frames=2)
        cur, prev = pushes[a["frame"]], pushes[max(a["frame"] - 1, 0)]
        st = self.vrt.ReprojectSettings().to_c(cur)
        g, _ = self.gbuffer(a["src"])
        frames = self.sequence_frames("g")
        self.keep += [cur, prev, st]
        ref = lambda x: C.byref(x) if x is not None else None
        return self.temporal(a, "reproject", H, W,
                             lambda hin, hout, res, mot: self.lib.vrt_reproject(self.engine.ctx, W, H, C.byref(cur), C.byref(prev), C.byref(st), g["color8"].data_ptr(),
                                                                                g["position"].data_ptr(), g["normal8"].data_ptr(), ref(hin), C.byref(hout),
                                                                                res.data_ptr(), mot.data_ptr()),
                             lambda: rc.run_definition(W, H, pushes, frames()))

    def h_vrt_upsample(self, a):
        (w, h), (TW, TH) = a["res"], a["target"]
        pushes = uc.pushes_of(self.vrt, self.oracle, sc.UPSAMPLE_PAIR, frames=2)
        cur, prev = pushes[a["frame"]], pushes[max(a["frame"] - 1, 0)]
        st = self.vrt.ReprojectSettings().to_c(cur)
        g, _ = self.gbuffer(a["src"])
        frames = self.sequence_frames("u")
        self.keep += [cur, prev, st]
        ref = lambda x: C.byref(x) if x is not None else None
        return self.temporal(a, "upsample", TH, TW,
                             lambda hin, hout, res, mot: self.lib.vrt_upsample(self.engine.ctx, w, h, TW, TH, C.byref(cur), C.byref(prev), C.byref(st), g["color8"].data_ptr(),
                                                                               g["position"].data_ptr(), g["normal8"].data_ptr(), ref(hin), C.byref(hout),
                                                                               res.data_ptr(), mot.data_ptr()),
                             lambda: uc.run_definition(sc.UPSAMPLE_PAIR, pushes, frames()))

    def h_vrt_reproject_camera(self, a):
        W, H = a["res"]
        made = _once((self.case.id, "cam frames"), lambda: (lambda cams: (cams, rcc.oracle_frames(self.vrt, self.oracle, 1, cams, W, H)))(
            rcc.cameras_of(self.vrt, self.oracle, a["model"], W, H, frames=2)))
        cams, frames = made
        f = a["frame"]
        cur, prev = cams[f], cams[max(f - 1, 0)]
        col, pos, nrm = (self.upload(f"{a['out']}.in{k}", x) for k, x in enumerate(frames[f]))         # (uploaded before the stall)
        st = self.cap.ReprojectSettings()
        self.lib.vrt_reproject_camera_settings_default(C.byref(cur), W, C.byref(st))
        self.vrt.ReprojectSettings().over(st)
        self.keep += [st]
        ref = lambda x: C.byref(x) if x is not None else None
        return self.temporal(a, "reproject_camera", H, W,
                             lambda hin, hout, res, mot: self.lib.vrt_reproject_camera(self.engine.ctx, W, H, C.byref(cur), C.byref(prev), C.byref(st), col.data_ptr(),
                                                                                       pos.data_ptr(), nrm.data_ptr(), ref(hin), C.byref(hout), res.data_ptr(),
                                                                                       mot.data_ptr()),
                             lambda: rcc.run_definition(W, H, cams, frames))

    def h_vrt_debug_denoise_redone(self, a):
        got = {}

        def launch():
            for p in a["passes"]:
                n = C.c_uint32()
                self.check(self.lib.vrt_debug_denoise_redone(self.engine.ctx, p, C.byref(n)))
                got[p] = int(n.value)

        def verify():
            print(f"case {self.case.id} on {self.kind}: pixels evaluated twice per pass {got}")
            if self.kind == "null":
                # a pass in the verified form that evaluated nothing twice would leave vrt_api_post.hip:150 unreached by every kind
                assert any(v > 0 for v in got.values()), (self.case.id, got, "no pass of the latest vrt_denoise counted a pixel")
                _redone[self.case.id] = dict(got)
            else:
                assert got == null_redone(self.vrt, self.oracle, self.case), (self.case.id, self.kind, got)
        return launch, verify


def null_redone(vrt, oracle, case):
    if case.id not in _redone:
        execute(vrt, oracle, case, "null")
    return _redone[case.id]


def execute(vrt, oracle, case, kind):
    """Runs the case; returns what was seen of the stall: {"behind": steps that started while it was pending, "stall_ms": its length
    on the device, "enqueue_ms": host time from its enqueue to the last step's} (null and side; own has no event to ask).  On side the count is held to the table's.  On null it is printed: the first use
    of a kernel or a helper stream in the process can hold the host until the null stream is idle (tests/stream_common.py)."""
    assert kind not in case.not_on
    side = torch.cuda.Stream() if kind == "side" else None
    # (null inside another case's side scope -- null_redone -- is still the null stream)
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        run = Run(vrt, oracle, case, kind)
        try:
            if kind == "null":
                assert torch.cuda.current_stream().cuda_stream == 0, "the control is the HIP null stream"
            if kind == "side":
                assert torch.cuda.current_stream() == side and side.cuda_stream != 0
            setup, steps, late = [], [], []
            for st in case.setup:
                setup.append(getattr(run, "h_" + st.name)(st.args))
            for st in case.steps:
                (late if st.name in sc.AFTER_THE_WAIT else steps).append(getattr(run, "h_" + st.name)(st.args))
            run.prepare_stall()
            torch.cuda.synchronize()
            for launch, _ in setup:
                launch()
            run.engine.synchronize()
            torch.cuda.synchronize()
            seen = None
            begun, ended = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if kind != "own":
                begun.record()
            t0 = time.perf_counter()
            run.stall()
            if kind != "own":
                ended.record()                   # on the context's stream: complete when the stall is
            pending = []
            for launch, _ in steps:
                if kind != "own":
                    pending.append(not ended.query())
                launch()
            t1 = time.perf_counter()
            run.engine.synchronize()
            if kind == "own":
                torch.cuda.synchronize()
            else:
                behind = pending.index(False) if False in pending else len(pending)
                seen = {"behind": behind, "stall_ms": begun.elapsed_time(ended), "enqueue_ms": 1e3 * (t1 - t0)}
                assert not any(pending[behind:]), pending
                print(f"case {case.id} on {kind}: {behind} of {len(pending)} steps started behind the stall ({seen['stall_ms']:.2f} ms; host {seen['enqueue_ms']:.2f} ms)")
                assert kind == "null" or behind == case.behind, (f"case {case.id} on {kind}: {behind} steps started while the stall was pending, the table says "
                                               f"{case.behind}; the stall took {seen['stall_ms']:.2f} ms, the host {seen['enqueue_ms']:.2f} ms")
            for launch, _ in late:
                launch()
            for _, verify in setup + steps + late:
                if verify is not None:
                    verify()
            if kind == "null":
                _rehearsed.add(case.id)
            return seen
        finally:
            run.close()


RUNS = [(k, c) for k in sc.KINDS for c in sc.CASES if k not in c.not_on]


@pytest.mark.parametrize("kind,case", RUNS, ids=[f"{c.id}-{k}" for k, c in RUNS])
def test_case_on_stream(vrt, oracle, case, kind):
    if kind != "null" and case.id not in _rehearsed:         # (a run of this kind alone: the control first, see stream_common.py)
        execute(vrt, oracle, case, "null")
    execute(vrt, oracle, case, kind)


def test_the_stall_outlasts_the_longest_sequences(vrt, oracle):
    """The cases in which no step waits (the tags sequence, the post chain, the copies) on a side stream: every step started while
    the stall was still pending (execute asserts the table's count for every case on side).  Prints how long the stall
    lasted on the device and how long the host took to enqueue stall and sequence: the margin DESIGN.md section 8 states for
    STALL_PASSES (not asserted: a ratio of two times on a shared machine)."""
    for case in (sc.E_TAGS2, sc.H, sc.I):
        if case.id not in _rehearsed:
            execute(vrt, oracle, case, "null")
        seen = execute(vrt, oracle, case, "side")
        print(f"case {case.id}: {seen['behind']} steps behind the stall; stall {seen['stall_ms']:.2f} ms, enqueue {seen['enqueue_ms']:.2f} ms")
        assert seen["behind"] == len([st for st in case.steps if st.name not in sc.AFTER_THE_WAIT])
