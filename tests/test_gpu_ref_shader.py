"""The HIP kernels against what the reference's own shaders, compiled as C++, computed (tests/golden/refshader_*.npz, recorded by
tests/golden/make_refshader_fixtures.py; the cases are those of tests/test_ref_shader_cpu.py).  The comparison is direct: the
recorded floats of the shader's outputs against the kernels' planes, by bit pattern, and the recorded floats through the target
formats' conversions (UNORM8 / SNORM8) against the 8-bit planes -- the oracle's renderer is not involved.
Only tests/golden/ is read.  Tolerance: 0."""
import ctypes as C

import numpy as np
import pytest

import ref_shader_common as rc
from ray_query_common import bricks_of
from test_ref_shader_cpu import fx

pytestmark = pytest.mark.gpu

PLANES = ("color8", "depth", "motion", "mask8", "position", "normal8", "color_f")


def _settings(vrt, rec, traversal=0, flags=0):
    v = rec["params"]
    st = vrt._capi.Settings()
    st.ao_samples = int(v[0]); st.ambient_intensity = float(v[1])
    st.light_dir[:] = [float(x) for x in v[2:5]]; st.light_intensity = float(v[5]); st.light_color[:] = [float(x) for x in v[6:10]]
    st.max_steps, st.ao_steps, st.max_bounces, st.shadows = 512, 64, 5, 1          # the shader's constants
    st.traversal, st.flags = traversal, flags
    return st


def _push(vrt, rec):
    return vrt._capi.Push.from_buffer_copy(rec["push"].tobytes())


def _mismatches(oracle, got, rec):
    """Planes of a kernel against the recorded shader outputs; {} when all equal."""
    bad = {}

    def chk(name, same):
        if not np.all(same):
            bad[name] = int((~np.asarray(same)).sum())
    chk("color_f", rc.same_bits(got["color_f"], rec["color"][..., :3]))
    chk("color8", got["color8"] == oracle.unorm8(rec["color"]))
    chk("depth", rc.same_bits(got["depth"], rec["depth"]))
    chk("motion", rc.same_bits(got["motion"], rec["motion"]))
    chk("mask8", got["mask8"] == oracle.unorm8(rec["mask"]))
    chk("position", rc.same_bits(got["position"][..., :3], rec["position"]) & (rc.bits(got["position"][..., 3:]) == 0))
    chk("normal8", (got["normal8"][..., :3] == oracle.snorm8(rec["normal"])) & (got["normal8"][..., 3:] == 0))
    return bad


@pytest.fixture(scope="module")
def scenes(vrt, engine):
    s = fx("scene")
    dense = vrt.VoxelScene.from_dense(engine, s["voxels"], s["palette"], sky=s["sky"], noise=s["noise"])
    grid, pool = bricks_of(s["voxels"])
    brick = vrt.VoxelScene.from_bricks(engine, grid, pool, s["palette"], sky=s["sky"], noise=s["noise"])
    yield dense, brick
    dense.destroy(); brick.destroy()


def _render(vrt, engine, scene, rec, st):
    gb = vrt.GeometryBuffer(engine, rc.W, rc.H, PLANES)
    fr = gb.to_c()
    push = _push(vrt, rec)
    vrt._capi.check(vrt.lib().vrt_render_geometry(engine.ctx, scene.handle, C.byref(push), C.byref(st), C.byref(fr), None))
    engine.synchronize()
    return gb.numpy()


@pytest.mark.parametrize("traversal", ["AUTO", "DENSE", "BITMASK", "JUMP", "DF", "DFJ"])
def test_render_geometry_equals_the_compiled_shader(vrt, oracle, engine, scenes, traversal):
    """vrt_render_geometry, one VRT_TRAVERSAL_* mode per test; inside, with and without VRT_FLAG_SPLIT_KERNELS, packed_bounces 0 / 1,
    ao_batch 0 / 1, on the four 72 x 44 cases (AO 0 / 1 / 4, frames 0 / 31 / 32 / 2^32 - 1, jitter, two lights, camera outside and
    inside): every plane equals the recorded shader output on every pixel."""
    trav = getattr(vrt._capi, "TRAVERSAL_" + traversal)
    for name in rc.GEOMETRY_CASES:
        rec = fx("geom_" + name)
        for flags in (0, 4):
            for packed in (0, 1):
                for batch in (0, 1):
                    with engine.options(packed_bounces=packed, ao_batch=batch):
                        got = _render(vrt, engine, scenes[0], rec, _settings(vrt, rec, trav, flags))
                    bad = _mismatches(oracle, got, rec)
                    assert not bad, (name, traversal, flags, packed, batch, bad)


def test_brick_scene_equals_the_compiled_shader(vrt, oracle, engine, scenes):
    """The same volume through vrt_scene_from_bricks (packed_bounces 2: the packed chain on brick scenes too, and 0)."""
    for name in rc.GEOMETRY_CASES:
        rec = fx("geom_" + name)
        for packed in (0, 2):
            with engine.options(packed_bounces=packed):
                got = _render(vrt, engine, scenes[1], rec, _settings(vrt, rec))
            bad = _mismatches(oracle, got, rec)
            assert not bad, (name, packed, bad)


def test_render_rays_equals_the_compiled_shader(vrt, oracle, engine, scenes):
    """vrt_render_rays fed the frame's own primary rays (origin camPos, the unit directions of the push block's ray table), dense and
    brick scene, ao_batch 0 / 1: the same planes."""
    import torch
    for name in rc.GEOMETRY_CASES:
        rec = fx("geom_" + name)
        push = rc.push_of(oracle, rec["push"])
        dirs = rc.ray_table(oracle, push).reshape(-1, 3)
        orig = np.tile(np.array(list(push.cam_pos)[:3], np.float32), (rc.W * rc.H, 1))
        o = torch.from_numpy(orig).to(engine.torch_device); d = torch.from_numpy(np.ascontiguousarray(dirs)).to(engine.torch_device)
        st = _settings(vrt, rec)
        for scene in scenes:
            for batch in (0, 1):
                gb = vrt.GeometryBuffer(engine, rc.W, rc.H, PLANES)
                fr = gb.to_c()
                with engine.options(ao_batch=batch):
                    vrt._capi.check(vrt.lib().vrt_render_rays(engine.ctx, scene.handle, rc.W, rc.H, C.c_void_p(o.data_ptr()),
                                                             C.c_void_p(d.data_ptr()), push.frame, C.byref(st), C.byref(fr)))
                    engine.synchronize()
                bad = _mismatches(oracle, gb.numpy(), rec)
                assert not bad, (name, scene is scenes[1], batch, bad)


def test_pick_pixels_equals_the_compiled_shader(vrt, oracle, engine, scenes):
    """vrt_pick_pixels on every third pixel (and the four corners): hit or miss, position by bit pattern, the int8 normal
    (-mask * rayStep) against the signs of the shader's normal."""
    idx = np.unique(np.concatenate([np.arange(0, rc.W * rc.H, 3), [0, rc.W - 1, rc.W * (rc.H - 1), rc.W * rc.H - 1]]))
    xy = np.stack([idx % rc.W, idx // rc.W], 1).astype(np.int32)
    for name in rc.GEOMETRY_CASES:
        rec = fx("geom_" + name)
        for scene in scenes:
            got = scene.pick(_push(vrt, rec), xy, 512)
            engine.synchronize()
            hit = rec["mask"][xy[:, 1], xy[:, 0]] != 0
            assert ((got["material"] != 0) == hit).all(), name
            assert 0.05 < hit.mean() < 0.95
            assert rc.same_bits(got["pos"][:, :3], rec["position"][xy[:, 1], xy[:, 0]]).all(), name
            assert (got["normal"] == np.sign(rec["normal"][xy[:, 1], xy[:, 0]]).astype(np.int8)).all(), name


@pytest.mark.parametrize("mode", [0, 1], ids=["canonical", "as_shipped"])
@pytest.mark.parametrize("w,h", rc.DENOISE_SIZES)
def test_denoise_equals_the_compiled_shader(vrt, oracle, engine, w, h, mode):
    """vrt_denoise with 1, 2 and 3 iterations of the default schedule: the last target equals the RGBA8 store of the recorded
    outColor of pass 0, 1, 2 (each recorded pass was fed the store of the one before, as the ping-pong targets are)."""
    import torch
    src, rec = fx(f"denoise_{w}x{h}_in"), fx(f"denoise_{w}x{h}_mode{mode}")
    dev = engine.torch_device
    color, normal, position = (torch.from_numpy(src[k].copy()).to(dev) for k in ("color", "normal", "position"))
    for it in (1, 2, 3):
        ds = vrt._capi.DenoiserSettings(it, 20.4, 1e-2, 1e-1, 2.0, mode)
        t0, t1 = torch.zeros_like(color), torch.zeros_like(color)
        res = C.c_void_p()
        vrt._capi.check(vrt.lib().vrt_denoise(engine.ctx, w, h, C.byref(ds), color.data_ptr(), normal.data_ptr(), position.data_ptr(),
                                             t0.data_ptr(), t1.data_ptr(), None, C.byref(res)))
        engine.synchronize()
        out = t0 if res.value == t0.data_ptr() else t1
        assert res.value in (t0.data_ptr(), t1.data_ptr())
        want = oracle.unorm8(rec[f"pass{it - 1}"])
        got = out.cpu().numpy()
        assert (got == want).all(), (it, int((got != want).sum()))


@pytest.mark.parametrize("sw,sh,tw,th", rc.BLIT_SIZES)
def test_blit_equals_the_compiled_shader(vrt, engine, sw, sh, tw, th):
    """vrt_blit on the size pairs and sources of test_blit_bit_exact against the RGBA8 store of the recorded outColor."""
    import torch
    k = rc.BLIT_SIZES.index((sw, sh, tw, th))
    want = fx("blit_a" if k % 2 == 0 else "blit_b")[f"codes_{sw}x{sh}_{tw}x{th}"]
    src = torch.from_numpy(rc.blit_source(sw, sh, th)).to(engine.torch_device)
    dst = torch.zeros((th, tw, 4), dtype=torch.uint8, device=engine.torch_device)
    vrt._capi.check(vrt.lib().vrt_blit(engine.ctx, src.data_ptr(), sw, sh, dst.data_ptr(), tw, th))
    engine.synchronize()
    assert (dst.cpu().numpy() == want).all()
