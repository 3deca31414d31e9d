"""What tests/test_gpu_streams.py (on the device) and tests/test_stream_cases_cpu.py (without one) share: the stages of the library
as sequences of C-ABI calls that are enqueued on the context's stream behind a busy device, on three kinds of stream.

  null   vrt.Engine(0) outside any stream scope: the HIP null stream, which orders itself against every blocking stream and
         carries every plain hipMemcpy -- the control, and what the session fixture `engine` gives every other GPU test
  own    vrt.Engine(0, use_torch_stream=False): the hipStreamNonBlocking stream vrt_ctx_create makes (bench.py's timed loops)
  side   a torch side stream made current around the constructor and every call of the case (distributed.py's second context)

The discipline of a case: every device buffer is made and filled with POISON; torch.cuda.synchronize(); SETUP steps (they may
wait); the stall; STEPS, without a synchronise by the caller; ONE vrt_ctx_synchronize; then the comparisons, bit for bit, with the
oracle and the numpy definitions.  A step is (name of a C-ABI function, arguments as data); names of buffers, scenes and volumes
are strings the executor resolves.  Steps that wait inside the library (an edit, vrt_scene_set_sky) are steps all the same: what
they do after their wait runs beside whatever the steps before left on the stream.

A missing dependency is a race: the stall makes the host run ahead of the device, so work that should have waited almost always
runs early enough to show; a passing run does not prove the ordering exists.  One stalled run per case is the test.

How far the host runs ahead is a property of the sequence, not only of the stall: several functions wait for c->stream on the host,
and the first of them in a sequence spends the stall.  They are the edits, vrt_scene_set_sky / _set_blue_noise, the scene builds,
vrt_scene_reserve_bricks, vrt_scene_download and vrt_debug_scene_state (at entry or at exit), and also launches of the geometry stage:
launch_tags when one of the context's two tag buffers has to grow (the first two launches of a fresh context, a larger batch later),
launch_records when the split form's records grow, next_table when the ring slot it takes is still in flight (the fifth table launch
waits for the first), and a panorama vrt_camera_rays while the previous one's kernel has not finished (pano_done).  So a case states
`behind`: how many of its steps START while the stall is still pending; the GPU test measures it with an event recorded right after
the stall and asserts it on the side kind (own has no event Python can ask; on null -- the control, which runs first in a process --
the count is printed only: there the first use of a kernel or of a helper stream in the process can hold the host until the null
stream's work is done, measured on an MI355X as a launch that took 6 to 10 ms of host time against 0.3 to 0.7 ms on later runs, and
a case run on side alone runs on null first for that reason).  Cases whose point is a helper stream (E, H) make the buffers in SETUP ("warm"
launches of the largest size) so that no launch of the sequence waits and every step is held; cases whose point is the first launch
of a fresh context (D) or a host wait of the library (A, B, C, F, G) hold what is enqueued up to and by the first step that waits."""
from collections import namedtuple

import numpy as np

import launch_shapes_common as lsc

KINDS = ("null", "own", "side")
POISON = lsc.POISON
STALL_BYTES, STALL_PASSES = 1 << 30, 16         # as _stall of tests/test_gpu_launch_shapes.py: a few milliseconds

Step = namedtuple("Step", "name args")
AFTER_THE_WAIT = ("vrt_debug_denoise_redone",)      # reads what the sequence left on the context: runs after the one synchronise


def S(name, **args):
    return Step(name, args)


class Case:
    """setup: steps before the stall; steps: the sequence behind it; imported: the shapes are launch_shapes_common's;
    not_on: {kind: reason} for a kind the case cannot run on; behind: how many steps start while the stall is pending (None: all
    that run before the one synchronise)."""

    def __init__(self, id, title, pins, setup, steps, imported=False, not_on=None, behind=None):
        self.id, self.title, self.pins, self.setup, self.steps = id, title, pins, list(setup), list(steps)
        self.imported, self.not_on = imported, dict(not_on or {})
        self.behind = behind if behind is not None else sum(st.name not in AFTER_THE_WAIT for st in self.steps)


# ---- volumes, skies, boxes: named here, built on demand --------------------------------------------------------------------------

def _sparse40(vrt):
    rng = np.random.default_rng(7)
    vol = ((rng.random((32, 24, 40)) < 0.04) * rng.integers(1, 200, (32, 24, 40))).astype(np.uint8)       # no metallic id
    vol[12:20, 8:16, 14:26] = 40
    return vol


def _world32(vrt):
    rng = np.random.default_rng(31)
    vol = (rng.random(lsc.BATCH_DIMS) < 0.05).astype(np.uint8) * rng.integers(1, 256, lsc.BATCH_DIMS).astype(np.uint8)
    vol[10:22, 12:20, 10:22] = 210
    return vol


def _cubes40(vrt):
    import reproject_common as rc
    return rc.scene_of(vrt, 1)[0]


VOLUMES = {"cubes32": lambda vrt: vrt.synthetic.floating_cubes(32, seed=1, count=40),          # render_rays_common's Scene A
           "sparse40": _sparse40,                                                              # 40 x 24 x 32
           "cubes48": lambda vrt: vrt.synthetic.floating_cubes(lsc.TAGS_DIMS[0], **lsc.TAGS_CUBES),        # 6^3 bricks
           "world32": _world32,
           "cubes40": _cubes40}
DIMS = {"cubes32": (32, 32, 32), "sparse40": (40, 24, 32), "cubes48": lsc.TAGS_DIMS, "world32": lsc.BATCH_DIMS, "cubes40": (40, 40, 40)}

_volumes = {}


def volume(vrt, name):
    """The named volume [z, y, x], built once and read-only."""
    if name not in _volumes:
        v = np.ascontiguousarray(VOLUMES[name](vrt), np.uint8)
        assert v.shape == DIMS[name][::-1]
        v.setflags(write=False)
        _volumes[name] = v
    return _volumes[name]


def sky(vrt, spec):
    """("gradient", w, h) or ("const", rgba) -> float32 [h, w, 4]"""
    if spec is None:
        return None
    if spec[0] == "gradient":
        return np.ascontiguousarray(vrt.synthetic.sky_gradient(spec[1], spec[2]), np.float32)
    return np.array([[list(spec[1])]], np.float32)


def noise(vrt, n):
    return None if n is None else vrt.synthetic.blue_noise_standin(n)


def box_ids(spec):
    """("random", seed, (w, h, d), share, metallic id or None) or ("zeros", (w, h, d)) -> uint8 [d, h, w]"""
    if spec[0] == "zeros":
        w, h, d = spec[1]
        return np.zeros((d, h, w), np.uint8)
    _, seed, (w, h, d), share, metal = spec
    rng = np.random.default_rng(seed)
    ids = ((rng.random((d, h, w)) < share) * rng.integers(1, 200, (d, h, w))).astype(np.uint8)
    if metal is not None:
        ids[d // 2, h // 2, :] = metal
    return ids


def apply_box(vol, lo, ids, size=None):
    """vol with the box written: the definition of vrt_scene_edit_box (ids: an array [d, h, w]) and of vrt_scene_fill_box (ids:
    one id for the box lo .. lo + size)."""
    out = np.array(vol)
    w, h, d = size if size is not None else ids.shape[::-1]
    out[lo[2]:lo[2] + d, lo[1]:lo[1] + h, lo[0]:lo[0] + w] = ids
    return out


def volume_after(vrt, steps, upto=None):
    """{scene name: volume} after the first `upto` steps (all of them: None) -- the numpy side of the edits of a sequence."""
    vols = {}
    for st in steps[:upto]:
        a = st.args
        if st.name in ("vrt_scene_from_dense", "vrt_scene_from_bricks"):
            vols[a["scene"]] = volume(vrt, a["volume"])
        elif st.name == "vrt_scene_edit_box":
            vols[a["scene"]] = apply_box(vols[a["scene"]], a["lo"], box_ids(a["ids"]))
        elif st.name == "vrt_scene_fill_box":
            vols[a["scene"]] = apply_box(vols[a["scene"]], a["lo"], a["id"], a["size"])
    return vols


# ---- the cases ------------------------------------------------------------------------------------------------------------------

BIG, RAGGED = (96, 64), (44, 28)                 # 44 x 28: the last wave of a row kernel holds 16 pixels, no tile is whole
SKY75, SKY11 = ("gradient", 7, 5), ("const", (0.2, 0.5, 0.9, 1.0))
DENSE_STATES = ("VOX", "DF", "OCC1", "OCC2", "OCC3", "CELLS")
BRICK_STATES = ("BENTRY", "BPOOL", "BFINE", "CELLS")


def _textured(scene="s"):
    return [S("vrt_scene_set_sky", scene=scene, sky=("gradient", 64, 32)), S("vrt_scene_set_blue_noise", scene=scene, noise=64)]


def _render(out, settings="default", res=BIG, scene="s", planes="gbuffer", **pose):
    return S("vrt_render_geometry", scene=scene, settings=settings, res=res, pose=pose, planes=planes, out=out)


A = Case("A", "scene lifecycle",
         "vrt_scene_set_sky / set_blue_noise: plain hipMemcpy behind their leading synchronise (vrt_api_scene.hip:33, :57); the build's cell "
         "list (:149); the hit-colour table made at the first primary-only launch and made again after each sky (vrt_api.hip:647-653); "
         "vrt_scene_download's plain D2H (vrt_api_scene.hip:468)",
         [],
         [S("vrt_scene_from_dense", scene="s", volume="cubes32"),
          _render("a0", "primary_only", frame=1),
          S("vrt_scene_set_sky", scene="s", sky=SKY75),
          S("vrt_scene_set_blue_noise", scene="s", noise=16),
          S("vrt_debug_sky_texels", scene="s", dirs=("panorama", (64, 32)), out="texels"),
          S("vrt_debug_spec", fn=2, pairs=("edges", 4099), out="atan2"),        # spec_common.FN_ATAN2; a last wave of three lanes
          _render("a1", frame=2, jitter=(0.25, -0.25)),
          S("vrt_scene_set_sky", scene="s", sky=SKY11),
          _render("a2", "primary_only", res=RAGGED, frame=3),
          _render("a3", res=RAGGED, frame=3),
          S("vrt_scene_download", scene="s")],
         behind=1)        # the build waits for its own copies: what it enqueued before that wait is what the stall holds

B = Case("B", "dense edits",
         "the edit's hipMemcpyAsync from caller memory; the cell list's plain hipMemcpy (vrt_api_scene.hip:149) between kernels; fields_for_counts "
         "building the count planes' fields after an edit dropped them",
         [S("vrt_scene_from_dense", scene="s", volume="sparse40")] + _textured() + [_render("w0", frame=1), _render("w1", frame=1)],
         [_render("b0", frame=1),
          S("vrt_scene_edit_box", scene="s", lo=(14, 6, 2), ids=("random", 3, (9, 10, 7), 0.5, 210)),        # the first metallic voxel
          _render("b1", frame=2),
          S("vrt_scene_fill_box", scene="s", lo=(0, 0, 0), size=(5, 4, 6), id=9),                           # a corner of the volume
          _render("b2", res=RAGGED, planes="debug", frame=3),
          S("vrt_debug_scene_state", scene="s", what=DENSE_STATES)],
         behind=2)        # b0 (tag buffers made in SETUP) and the edit, which waits for b0 at entry

C = Case("C", "brick edits",
         "ptr_dev and list_dev (plain hipMemcpy between kernels, vrt_api_edit.hip:203, :218); the device-to-device pool copies of "
         "vrt_scene_reserve_bricks (:380-:381); brick_upload_cells (:118); the build's cell list (vrt_api_scene.hip:334)",
         [],
         [S("vrt_scene_from_bricks", scene="s", volume="cubes48")] + _textured() +
         [_render("c0", frame=1),
          S("vrt_scene_reserve_bricks", scene="s", extra=6),
          S("vrt_scene_fill_box", scene="s", lo=(20, 20, 0), size=(8, 8, 3), id=215),                       # new bricks, metallic
          _render("c1", frame=2),
          S("vrt_scene_edit_box", scene="s", lo=(16, 16, 0), ids=("zeros", (8, 8, 8))),                     # a brick empties: its slot is free
          S("vrt_scene_fill_box", scene="s", lo=(41, 42, 1), size=(3, 3, 3), id=7),                         # ... and is taken again
          _render("c2", frame=3),
          S("vrt_debug_scene_state", scene="s", what=BRICK_STATES)],
         behind=1)

_FRESH = [S("vrt_scene_from_dense", scene="s", volume="cubes32")] + _textured()
D1 = Case("D1", "lazy state first: count planes", "fields_for_counts as the first launch of a context",
          _FRESH, [_render("d", res=RAGGED, planes="debug", frame=1)], behind=1)
D2 = Case("D2", "lazy state first: split kernels", "launch_records' buffers as the first launch of a context",
          _FRESH, [_render("d", "split", frame=1)], behind=1)
D3 = Case("D3", "lazy state first: hit table", "the hit-colour table (vrt_api.hip:647-653) as the first launch of a context",
          _FRESH, [_render("d", "primary_only", frame=1)], behind=1)

def _ring_batch(out, k=0):
    return S("vrt_render_geometry_batch", scene="s", settings="default", res=lsc.BATCH_RES, poses=(k * lsc.RING_N, (k + 1) * lsc.RING_N), out=out)


_RING = [_ring_batch(f"r{k}", k) for k in range(lsc.RING_LAUNCHES)]
SLOTS_RANKS, SLOTS_STRIP = 2, 16                 # 32 rows: one strip of 16 rows per rank
E_RING = Case("E-ring", "table ring",
              "upload_stream with tab_uploaded / tab_consumed: the fifth table launch takes the ring slot of the first",
              [S("vrt_scene_from_dense", scene="s", volume="world32")] + _textured() + [_ring_batch("w0"), _ring_batch("w1")],
              _RING + [S("vrt_render_geometry_slots", scene="s", settings="default", res=lsc.BATCH_RES, poses=(0, lsc.RING_N),
                         ranks=SLOTS_RANKS, strip_rows=SLOTS_STRIP, out="slots")], imported=True,
              behind=lsc.TAB_RING + 1)       # the two warm launches took ring slots 0 and 1 and are done; r0 .. r3 take 2, 3, 0, 1 and are
                                             # held; r4 starts behind the stall and waits on the host for r0 (slot 2): that wait is the subject


def _tags_steps():
    out = []
    for k, (kind, what, shard) in enumerate(lsc.TAGS_SEQ):
        if kind == "single":
            out.append(S("vrt_render_geometry", scene="s", settings="default_ao2", res=lsc.TAGS_RES, tags_pose=what, shard=shard,
                         planes="launch", out=f"t{k}"))
        else:
            out.append(S("vrt_render_geometry_batch", scene="s", settings="default_ao2", res=lsc.TAGS_RES, tags_poses=what, out=f"t{k}"))
    return out


_TAGS_LARGEST = max((w for k, w, _ in lsc.TAGS_SEQ if k == "batch"), key=lambda w: w[1] - w[0])


def _tags_case(value):
    return Case(f"E-tags{value}", f"tile tags, tags_async = {value}",
                "tag_stream with tag_done / tag_read against c->stream; launch_tags' hipMemcpyAsync from a vector that dies (vrt_api.hip:569-570)",
                # both tag buffers made at the largest batch's size while tags_async is 0; the option is set last, so the FIRST launch of
                # the sequence is the one that makes the tag stream -- behind everything the stall left on c->stream (defect (b))
                [S("vrt_scene_from_dense", scene="s", volume="cubes48")] + _textured() +
                [S("vrt_render_geometry_batch", scene="s", settings="default_ao2", res=lsc.TAGS_RES, tags_poses=_TAGS_LARGEST, out=f"w{k}") for k in range(2)] +
                [S("vrt_ctx_set_option", option="tags_async", value=value)],
                _tags_steps(), imported=True)


E_TAGS0, E_TAGS2 = _tags_case(0), _tags_case(2)

PANO_AT = (16.5, 30.5, 16.5)                     # render_rays_common.PANORAMA_AT: inside cubes32
PERSPECTIVE = dict(frame=3, jitter=(0.31, -0.23))        # camera_push's pose of cubes32, tan_half = 1: the renderer's own camera
_F = [S("vrt_camera_rays", model="panorama", at=PANO_AT, res=(64, 32), out="p0"),
      S("vrt_camera_rays", model="panorama", at=(1.0, 2.0, 3.0), res=(96, 40), out="p1"),         # the tables grow while p0 is queued
      S("vrt_camera_rays", model="panorama", at=PANO_AT, res=(64, 32), out="p2"),
      S("vrt_camera_rays", model="perspective", dims="cubes32", pose=PERSPECTIVE, res=RAGGED, out="pp"),
      S("vrt_camera_rays", model="orthographic", res=RAGGED, out="po")]                           # render_rays_common.ORTHO
F = Case("F", "panorama tables", "the pinned image of the panorama's tables and the pano_done wait (vrt_api_rays.hip:28-38)", [], _F,
         behind=2)        # p0 is held; p1 starts behind the stall and waits on the host for p0's kernel before it refills the tables
G = Case("G", "queries and shaded rays", "k_query / k_shade behind the kernel that makes their rays, no host wait in between",
         _FRESH,
         _F + [S("vrt_trace_rays", scene="s", rays="p2", max_steps=512, out="trace"),
               S("vrt_occluded_rays", scene="s", rays="po", max_steps=512, out="occ"),
               S("vrt_render_rays", scene="s", rays="pp", res=RAGGED, frame=PERSPECTIVE["frame"], settings="default", out="shaded"),
               S("vrt_pick_pixels", scene="s", dims="cubes32", pose=PERSPECTIVE, res=RAGGED, max_steps=512, out="pick")],
         behind=2)        # as F; the queries run behind the kernels that make their rays, with no host wait between the two

UPSAMPLE_PAIR = (64, 43, 96, 64)                 # upsample_common.PAIRS[0]: 1.5x
CAM_MODEL = "perspective"
BLIT_TARGET = (120, 80)


def _post_steps():
    st = [S("vrt_render_geometry", scene="s", settings="default_ao2", res=BIG, seq=("reproject", 0), planes="gbuffer", out="g0"),
          S("vrt_denoise", src="g0", res=BIG, iterations=2, mode=1, out="den1"),
          S("vrt_denoise", src="g0", res=BIG, iterations=2, mode=0, out="den0"),                  # the latest call: its counts are read
          S("vrt_accumulate", src="den1", res=BIG, acc="acc", reset=1),
          S("vrt_accumulate", src="den0", res=BIG, acc="acc", reset=0),
          S("vrt_resolve", acc="acc", res=BIG, frames=2, out="mean"),
          S("vrt_blit", src="mean", res=BIG, target=BLIT_TARGET, out="blit"),
          S("vrt_reproject", src="g0", res=BIG, frame=0, out="rp0"),
          S("vrt_render_geometry", scene="s", settings="default_ao2", res=BIG, seq=("reproject", 1), planes="gbuffer", out="g1"),
          S("vrt_reproject", src="g1", res=BIG, frame=1, out="rp1")]
    for f in range(2):
        st += [S("vrt_render_geometry", scene="s", settings="default_ao2", res=UPSAMPLE_PAIR[:2], seq=("upsample", f), planes="gbuffer", out=f"u{f}"),
               S("vrt_upsample", src=f"u{f}", res=UPSAMPLE_PAIR[:2], target=UPSAMPLE_PAIR[2:], frame=f, out=f"up{f}")]
    st += [S("vrt_reproject_camera", model=CAM_MODEL, res=RAGGED, frame=f, out=f"rc{f}") for f in range(2)]
    return st


H = Case("H", "post chain",
         "the denoiser's count buffer made and cleared on c->stream; vrt_debug_denoise_redone's plain D2H (vrt_api_post.hip:150); the "
         "history pairs handed from frame to frame on one stream",
         [S("vrt_scene_from_dense", scene="s", volume="cubes40")] + _textured() + [S("vrt_ctx_set_option", option="denoise_count", value=1)] +
         [S("vrt_render_geometry", scene="s", settings="default_ao2", res=BIG, seq=("reproject", 0), planes="gbuffer", out=f"w{k}") for k in range(2)],
         _post_steps() + [S("vrt_debug_denoise_redone", passes=(0, 1))])
# (vrt_debug_denoise_redone waits for the stream itself; the executor calls it after the one synchronise, as the last step)

COPY_N, COPY_BPP = 65, 4                        # the 65th image: a second launch of the batch forms (lsc.ROWS_BATCH = 64)
COPY_SHARD = lsc.copy_shards(2)[1]                # (rank, nranks) = (1, 2)
_COPY = dict(res=(lsc.COPY_W, lsc.COPY_H), bpp=COPY_BPP, strip_rows=lsc.COPY_STRIP, halo=lsc.COPY_HALO)
I = Case("I", "strip and halo copies",
         "the pointer tables the four batch forms upload per launch of 64 images, and the single forms, on a non-null stream; the shards "
         "are launch_shapes_common.copy_shards(): a different one per image",
         [],
         [S("vrt_pack_rows", src="full", shard=COPY_SHARD, out="packed1", **_COPY),
          S("vrt_unpack_rows", src="packed1", shard=COPY_SHARD, out="full1", **_COPY),
          S("vrt_pack_halo", src="full", shard=COPY_SHARD, direction=1, out="halo1", **_COPY),
          S("vrt_unpack_halo", src="halo1", shard=COPY_SHARD, direction=1, out="fullh1", **_COPY),
          S("vrt_pack_rows_batch", src="fulls", n=COPY_N, shard=COPY_SHARD, out="packed", **_COPY),        # one shard for all images
          S("vrt_unpack_rows_batch", src="packed", n=COPY_N, shard=COPY_SHARD, out="unpacked", **_COPY),
          S("vrt_pack_halo_batch", src="fulls", n=COPY_N, direction=-1, out="halos", **_COPY),              # copy_shards(n): one per image
          S("vrt_unpack_halo_batch", src="halos", n=COPY_N, direction=-1, out="unhalos", **_COPY)], imported=True)
# (each unpack reads what the pack before it wrote, with no host wait between the two)

CASES = [A, B, C, D1, D2, D3, E_RING, E_TAGS0, E_TAGS2, F, G, H, I]
BY_ID = {c.id: c for c in CASES}

# Every vrt_* function that takes a vrt_ctx* is named by a step above or here, never both (tests/test_stream_cases_cpu.py).
NOT_STREAMED = {
    "vrt_ctx_destroy": "host only: ends the context; every test's finally calls it",
    "vrt_ctx_set_stream": "host only: binds the stream; the null and side engines are made by it",
    "vrt_ctx_synchronize": "synchronises and touches no device memory: the one wait of every case",
    "vrt_ctx_get_option": "host only",
    "vrt_ctx_set_timing": "host only: a flag",
    "vrt_last_timings": "synchronises two events and touches no device memory",
    "vrt_device_info": "host only",
    "vrt_device_alloc": "hipMalloc, no stream; the own kind's stall buffer is made by it",
    "vrt_device_free": "synchronises, then hipFree; the own kind's stall buffer goes through it",
    "vrt_memset": "the own kind's stall itself: hipMemsetAsync on c->stream",
    "vrt_memcpy_h2d": "hipMemcpyAsync on c->stream and its synchronise, nothing else",
    "vrt_memcpy_d2h": "hipMemcpyAsync on c->stream and its synchronise, nothing else",
    "vrt_scene_load_vox_file": "host only up to vrt_scene_from_dense (case A)",
    "vrt_scene_load_vox_mem": "host only up to vrt_scene_from_dense (case A)",
    "vrt_scene_set_sky_file": "host only up to vrt_scene_set_sky (case A)",
    "vrt_scene_set_blue_noise_file": "host only up to vrt_scene_set_blue_noise (case A)",
    "vrt_scene_trim": "hipDeviceSynchronize, then frees",
    "vrt_scene_free": "synchronises, then frees; every case ends with it",
    "vrt_debug_brick_counts": "diagnostic of a counting build of the library; synchronises",
    "vrt_comm_init_rank": "RCCL, needs a node",
    "vrt_gather_strips": "RCCL, needs a node",
}


def all_steps():
    return [(c, st) for c in CASES for st in c.setup + c.steps]
