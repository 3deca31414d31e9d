"""The oracle against the reference's own shaders compiled as C++ (oracle/ref_shader/: voxel_volume.frag, denoiser.frag, blit.frag
behind a vector header that owns exactly the numeric choices of DESIGN.md section 3).  What the compiled shaders computed for the
cases of ref_shader_common.py is recorded in tests/golden/refshader_*.npz; where oracle/_ref/libvrt_refshader.so is present (or can
be built: the reference tree lies beside the repository) the recordings are re-derived live and must be equal, otherwise the
recordings alone carry the tests.  Tolerance everywhere: 0 -- floats are compared by bit pattern, codes as integers.

One thing is compared modulo the sign of zero: the normal's floats.  The shader's `vec3(mask) * -vec3(rayStep)` gives -0 on the
axes the ray did not cross with a positive step, the oracle writes +0 there; no output can show it (the normal reaches SNORM8,
`pos + normal * 0.01`, dot products that are clamped by max(., 0.0), and atan / asin that treat -0 as 0), and colour, depth and
position, which are computed from it, are equal bit for bit."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import ref_shader_common as rc

_cache = {}


def fx(name):
    if name not in _cache:
        with np.load(os.path.join(rc.GOLDEN, f"refshader_{name}.npz")) as z:
            _cache[name] = {k: z[k] for k in z.files}
        for a in _cache[name].values():
            a.setflags(write=False)
    return _cache[name]


def _scene(oracle, voxels="voxels"):
    s = fx("scene")
    return oracle.OracleScene(s[voxels], s["palette"], sky=s["sky"], noise=s["noise"])


def _oracle_frame(oracle, osn, rec):
    """The oracle's planes for a recorded case, and its float normals (vo_trace_ray of every primary ray)."""
    push, par = rc.push_of(oracle, rec["push"]), rc.params_of(oracle, rec["params"])
    exp = oracle.render(osn, push, par)
    w, h = push.screen_size[0], push.screen_size[1]
    normal = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            s, d = oracle.primary_ray(push, x, y)
            hit = oracle.trace_ray(osn, s, d)
            if hit.material:
                normal[y, x] = list(hit.normal)
    return push, par, exp, normal


def _differences(oracle, rec, exp, normal):
    """(H, W) bool per output: where the oracle differs from the recorded shader output."""
    d = {"color_f": ~rc.same_bits(rec["color"][..., :3], exp["color_f"]).all(-1),
         "alpha": rc.bits(rec["color"][..., 3]) != 0,
         "depth": ~rc.same_bits(rec["depth"], exp["depth"]),
         "motion": (rc.bits(rec["motion"]) != 0).any(-1) | (rc.bits(exp["motion"]) != 0).any(-1),
         "position": ~rc.same_bits(rec["position"], exp["position"][..., :3]).all(-1) | (rc.bits(exp["position"][..., 3]) != 0),
         "normal": ~rc.same_bits(rc.canonical_zero(rec["normal"]), normal).all(-1),
         "color8": (oracle.unorm8(rec["color"]) != exp["color8"]).any(-1),
         "mask8": oracle.unorm8(rec["mask"]) != exp["mask8"],
         "normal8": (oracle.snorm8(rec["normal"]) != exp["normal8"][..., :3]).any(-1) | (exp["normal8"][..., 3] != 0)}
    return d


# ---- the shim's volume fetch ------------------------------------------------------------------------------------------------------

def test_volume_texel_is_the_inverse_of_the_shaders_coordinate():
    """texture(scene, vec3(pos) / vec3(bounds)) returns texel rint(uvw * size): rint(float(p) / float(n) * float(n)) == p for every
    0 <= p < n <= 4096 (fp32 division and multiplication, round half to even)."""
    for n in range(1, 4097):
        p = np.arange(n, dtype=np.float32)
        back = np.rint((p / np.float32(n)) * np.float32(n))
        assert back.dtype == np.float32 and (back == p).all(), n


# ---- the recordings are what the compiled shaders compute ----------------------------------------------------------------------

def test_recordings_equal_the_live_shaders(oracle):
    """Where the library is present: every array of every refshader_*.npz, inputs included, equals what make_refshader_fixtures.record()
    derives now from the reference's shader text."""
    if oracle.refshader() is None:
        pytest.skip("oracle/_ref/libvrt_refshader.so is absent and the reference is not here to build it from")
    spec = importlib.util.spec_from_file_location("make_refshader_fixtures", os.path.join(rc.GOLDEN, "make_refshader_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    live = mod.record()
    on_disk = {f[len("refshader_"):-4] for f in os.listdir(rc.GOLDEN) if f.startswith("refshader_") and f.endswith(".npz")}
    assert on_disk == set(live)
    for name, arrays in live.items():
        rec = fx(name)
        assert set(rec) == set(arrays), name
        for k, a in arrays.items():
            a = np.asarray(a)
            assert rec[k].dtype == a.dtype and rec[k].shape == a.shape and rec[k].tobytes() == a.tobytes(), (name, k)


def test_recorded_inputs_are_the_cases(oracle):
    """The inputs in the files are the ones ref_shader_common.py builds (the GPU tests and the statistics below use either)."""
    vol, pal, sky, noise = rc.scene()
    s = fx("scene")
    for k, a in (("voxels", vol), ("palette", pal), ("sky", sky), ("noise", noise), ("face_voxels", rc.face_scene())):
        assert s[k].tobytes() == a.tobytes(), k
    assert (vol[0] == 0).all() and (vol[-1] == 0).all() and (vol[:, 0] == 0).all() and (vol[:, -1] == 0).all()
    assert (vol[:, :, 0] == 0).all() and (vol[:, :, -1] == 0).all()                     # the outer shell is empty
    assert vol.shape == rc.DIMS[::-1] and len(set(rc.DIMS)) == 3
    assert sky.shape[:2] == (19, 37) and noise.shape[:2] == (48, 80)                    # not powers of two, not 512 x 512
    for name in rc.GEOMETRY_CASES:
        push, par = rc.geometry_case(oracle, name)
        assert fx("geom_" + name)["push"].tobytes() == bytes(push)
        assert (fx("geom_" + name)["params"] == rc.params_vector(par)).all()
    assert {c[2] for c in rc.GEOMETRY_CASES.values()} == {0, 1, 4}
    assert {c[3] for c in rc.GEOMETRY_CASES.values()} == {0, 31, 32, 2 ** 32 - 1}
    assert all(c[4] != (0.0, 0.0) for c in rc.GEOMETRY_CASES.values())
    assert rc.LIGHT_DOWN[1] < 0 < rc.LIGHT_UP[1]
    for w, h in rc.DENOISE_SIZES:
        for k, a in zip(("color", "normal", "position"), rc.denoise_inputs(w, h)):
            assert fx(f"denoise_{w}x{h}_in")[k].tobytes() == a.tobytes()
            assert np.isfinite(a).all()


# ---- geometry ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(rc.GEOMETRY_CASES))
def test_geometry_equals_the_compiled_shader(oracle, name):
    """oracle.render == main() of voxel_volume.frag on all 72 x 44 pixels: colour (alpha 0), depth, motion, position by bit pattern,
    the normal's floats by bit pattern modulo the sign of zero, and color8 / mask8 / normal8 after the oracle's unorm8 / snorm8.
    No exclusion mask: no primary direction has a zero component (checked from the ray table) and the volume's shell is empty."""
    rec = fx("geom_" + name)
    osn = _scene(oracle)
    push, par, exp, normal = _oracle_frame(oracle, osn, rec)
    dirs = rc.ray_table(oracle, push)
    assert (dirs != 0).all() and all(c != 0 for c in par.light_dir)
    assert np.isfinite(rec["color"]).all() and np.isfinite(rec["position"]).all()
    bad = {k: int(v.sum()) for k, v in _differences(oracle, rec, exp, normal).items() if v.any()}
    assert not bad, (name, bad)
    assert ((rec["mask"] != 0) == (exp["hit_id"] != 0)).all()


def test_geometry_cases_are_not_trivial(oracle):
    """Per case: hits and misses >= 5 % each, pixels whose chain bounces >= 10 %, shadowed hits >= 5 % of the frame, lit hits >= 5 %
    under the light above the horizon and >= 1 % under the one below it (there every upward face shadows itself).
    Over the cases: chains of 0, 1 and 5 bounces, chains that end in the sky, and chains of five metallic hits (reflection 0)."""
    osn = _scene(oracle)
    metallic = fx("scene")["palette"][:, 4]
    lengths, sky_end, all_metal = set(), 0, 0
    for name in rc.GEOMETRY_CASES:
        push, par = rc.geometry_case(oracle, name)
        hit, chain, end, shadowed = rc.chain_stats(oracle, osn, push, par, metallic)
        assert 0.05 <= hit.mean() <= 0.95, (name, hit.mean())
        assert (chain > 0).mean() >= 0.10, (name, (chain > 0).mean())
        lit_min = 0.05 if par.light_dir[1] > 0 else 0.01
        assert shadowed.mean() >= 0.05 and (hit & ~shadowed).mean() >= lit_min, (name, shadowed.mean(), (hit & ~shadowed).mean())
        lengths |= set(np.unique(chain).tolist())
        sky_end += int((end == "sky").sum())
        all_metal += int(((chain == 5) & (end == "metal")).sum())
    assert {0, 1, 5} <= lengths and sky_end >= 100 and all_metal >= 8, (lengths, sky_end, all_metal)


# ---- the two documented divergences, each exactly what section 3 says ---------------------------------------------------------------

def test_axis_parallel_rays_literal_zero_times_inf(oracle):
    """9.4-I.  The 9 x 7 frame along +z: the centre column's rays have dir.x == 0, the centre row's dir.y == 0, the centre pixel both.
    Literal GLSL makes sideDist NaN on such an axis at the first step (vec3(mask) * deltaDist = 0 * inf); the oracle's select
    semantics keep it at +inf.
      one zero component: the march is the same (NaN <= x is false like inf <= x, and min ignores the NaN), so hit or miss (outMask)
        agrees with the oracle; the compiled shader's hit position is NaN in every component (0 * (NaN - inf) under the length),
        and with it depth; the oracle's are finite.
      two zero components (the ray parallel to an axis): min(NaN, NaN) is NaN, every comparison is false, the literal march never
        leaves its first voxel and reports a miss with position 0 where the oracle hits after 7 fetches.
    Everywhere else (off the centre row and column, and on their misses) every output is equal as in the general cases."""
    rec = fx("geom_axis")
    osn = _scene(oracle)
    push, par, exp, normal = _oracle_frame(oracle, osn, rec)
    nzero = (rc.ray_table(oracle, push) == 0).sum(-1)
    w, h = rc.AXIS_RES
    expect = np.zeros((h, w), int); expect[h // 2, :] += 1; expect[:, w // 2] += 1
    assert (nzero == expect).all()
    hit = exp["hit_id"] != 0
    one, two = (nzero == 1) & hit, (nzero == 2) & hit
    assert one.sum() >= 8 and two.sum() == 1 and ((nzero == 0) & hit).sum() >= 8
    assert (oracle.unorm8(rec["mask"]) == exp["mask8"])[~two].all() and ((rec["mask"] != 0) == hit)[~two].all()
    assert np.isnan(rec["position"][one]).all() and np.isnan(rec["depth"][one]).all()
    assert np.isfinite(exp["position"]).all() and np.isfinite(exp["depth"]).all() and np.isfinite(exp["color_f"]).all()
    assert (rec["mask"][two] == 0).all() and (rec["position"][two] == 0).all() and (exp["steps_primary"][two] == 7).all()
    for k, v in _differences(oracle, rec, exp, normal).items():
        assert not (v & ~(one | two)).any(), k


def test_first_voxel_solid_mask(oracle):
    """9.4-A.  A solid outer face seen from outside, 40 x 28, no zero direction component.  The shader leaves RayHitInternal.mask
    unwritten when the first sampled voxel is solid; compiled with zero initialisation it is (0, 0, 0), the oracle's rule A makes it
    the box-entry axes.  The two differ only on the pixels whose first sampled voxel is solid (steps_primary == 1), the material (hit
    or miss) agrees everywhere, and on those pixels the compiled shader's outputs are exactly what mask = 0 means: normal 0,
    position = the march's start point (the oracle's p0: d = length(0) = 0), depth = length(p0 - camPos).
    (mask enters the normal and, through d = length(mask * (sideDist - deltaDist)), the position: with the entry axis set d is the
    0.1 that boxIntersection advanced, so the oracle's position and depth lie 0.1 further along the ray than the zero mask's.)"""
    rec = fx("geom_face")
    osn = _scene(oracle, "face_voxels")
    push, par, exp, normal = _oracle_frame(oracle, osn, rec)
    assert (rc.ray_table(oracle, push) != 0).all()
    first = (exp["steps_primary"] == 1) & (exp["hit_id"] != 0)
    assert first.sum() >= 200 and ((exp["hit_id"] != 0) & ~first).sum() >= 50 and (exp["hit_id"] == 0).sum() >= 20
    assert (exp["hit_mask"][first] != 0).all()                     # rule A gave them an entry axis
    assert (oracle.unorm8(rec["mask"]) == exp["mask8"]).all()      # material: hit or miss agrees everywhere
    diff = _differences(oracle, rec, exp, normal)
    for k, v in diff.items():
        assert not (v & ~first).any(), k                           # nothing differs anywhere else
    cam = np.array(list(push.cam_pos)[:3], np.float32)
    ys, xs = np.nonzero(first)
    for y, x in zip(ys, xs):
        s, d = oracle.primary_ray(push, x, y)
        p0 = np.array(list(oracle.trace_ray(osn, s, d).p0), np.float32)
        assert rc.same_bits(rec["position"][y, x], p0).all(), (x, y)
        v = p0 - cam
        depth = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        assert rc.same_bits(rec["depth"][y, x], depth), (x, y)
        assert (rec["normal"][y, x] == 0).all()
    assert diff["position"][first].all() and diff["depth"][first].all() and diff["normal"][first].all()


# ---- denoiser -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [0, 1], ids=["canonical", "as_shipped"])
@pytest.mark.parametrize("w,h", rc.DENOISE_SIZES)
def test_denoiser_equals_the_compiled_shader(oracle, w, h, mode):
    """Passes 0, 1, 2 of the default schedule (step widths 1, 3, 5; pass 0 with phi = +inf), each fed the RGBA8 store of the pass before:
    outColor by bit pattern before the store, by code after.  Canonical reads the two uniform arrays with their intended strides, as
    shipped with std140's 16 bytes over the tight upload -- the same shader text."""
    src = fx(f"denoise_{w}x{h}_in")
    rec = fx(f"denoise_{w}x{h}_mode{mode}")
    color = src["color"]
    for i in range(3):
        p = oracle.denoise_pass_params(i)
        assert p.step_width == 2 * i + 1
        got = oracle.denoise_pass_f(color, src["normal"], src["position"], p, mode)
        want = rec[f"pass{i}"]
        assert np.isfinite(want).all()
        assert rc.same_bits(got, want).all(), (i, int((~rc.same_bits(got, want)).sum()))
        codes = np.zeros((h, w, 4), np.uint8)
        oracle.lib().vo_denoise_pass(color.ctypes.data, src["normal"].ctypes.data, src["position"].ctypes.data, codes.ctypes.data,
                                     w, h, p, mode, 0, h)
        assert (codes == oracle.unorm8(want)).all(), i
        color = np.ascontiguousarray(codes)
    assert (color != src["color"]).mean() > 0.5
    if mode == 0:
        assert (oracle.unorm8(rec["pass2"]) != oracle.unorm8(fx(f"denoise_{w}x{h}_mode1")["pass2"])).mean() > 0.2


# ---- blit -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sw,sh,tw,th", rc.BLIT_SIZES)
def test_blit_equals_the_compiled_shader(oracle, sw, sh, tw, th):
    """The size pairs and sources of test_blit_bit_exact: outColor by bit pattern (through the recorded SHA-256 of the float image:
    the images themselves would not fit the fixture size), and by code after the store."""
    k = rc.BLIT_SIZES.index((sw, sh, tw, th))
    rec = fx("blit_a" if k % 2 == 0 else "blit_b")
    src = rc.blit_source(sw, sh, th)
    tag = f"{sw}x{sh}_{tw}x{th}"
    assert hashlib.sha256(oracle.blit_f(src, tw, th).tobytes()).digest() == rec["sha256_" + tag].tobytes()
    assert (oracle.blit(src, tw, th) == rec["codes_" + tag]).all()
