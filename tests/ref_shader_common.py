"""Cases of the pin to the reference's shaders compiled as C++ (oracle/ref_shader/): shared by tests/golden/make_refshader_fixtures.py,
tests/test_ref_shader_cpu.py and tests/test_gpu_ref_shader.py.  Everything here is numpy and the oracle's ctypes structs: the inputs
of a case are recorded in tests/golden/refshader_*.npz beside the compiled shader's outputs, so the tests need neither the
reference nor the library built from it."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H = 72, 44                                   # ragged against 8 x 8 blocks and 32 x 8 spans
DIMS = (40, 24, 32)                             # x, y, z: not a cube, outer one-voxel shell empty
SHADER_PLANES = ("color", "depth", "motion", "mask", "position", "normal")


def scene():
    """voxels[z, y, x], palette (256, 5), sky (19, 37, 4) float32, noise (48, 80, 4) uint8: a sparse random volume (ids >= 128
    metallic) between a metallic floor and a partial metallic ceiling, so that bounce chains of every length occur -- between floor and
    ceiling all five bounces are metal (reflection 0), past the ceiling's edge chains end in the sky."""
    rng = np.random.default_rng(20240)
    X, Y, Z = DIMS
    vol = np.zeros((Z, Y, X), np.uint8)
    inner = (rng.random((Z - 2, Y - 2, X - 2)) < 0.035)
    vol[1:-1, 1:-1, 1:-1] = inner * rng.integers(1, 256, inner.shape).astype(np.uint8)
    vol[2:Z // 2 + 4, 2, 2:-2] = 200            # floor (metal) under the front part
    vol[2:-2, Y - 4, 2:X // 2] = 201            # half a ceiling (metal)
    vol[Z - 3, 3:Y - 4, 2:-2] = 77              # a plain back wall
    pal = np.zeros((256, 5), np.float32)
    pal[:, :3] = rng.random((256, 3)).astype(np.float32) * np.float32(0.8) + np.float32(0.1)
    pal[:, 3] = 1.0
    pal[128:, 4] = 0.75
    sky = (rng.random((19, 37, 4)).astype(np.float32) * np.float32(1.5)).astype(np.float32)
    sky[:, :, 3] = 1.0
    noise = rng.integers(0, 256, (48, 80, 4), dtype=np.uint8)
    return vol, pal, sky, noise


def face_scene():
    """9.4-A: a solid outer face (z = 0 plane of a 16 x 12 x 10 volume, with a hole) seen from outside."""
    vol = np.zeros((10, 12, 16), np.uint8)
    vol[0, :, :] = 9
    vol[0, 4:8, 5:11] = 0
    vol[6, 2:10, 3:13] = 140
    return vol


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def make_push(oracle, dims, res, pos, look, frame, jitter, focal=1.0):
    """A push block from a position and a viewing direction: an orthonormal basis, cam_right / cam_up scaled by 1 / focal."""
    d = _unit(look)
    r = _unit(np.cross(d, (0.0, 1.0, 0.0)))
    u = np.cross(r, d)
    p = oracle.Push()
    p.cam_pos[:] = [*map(float, pos), 1.0]
    p.cam_dir[:] = [*map(float, d), 0.0]
    p.cam_right[:] = [*map(float, r / focal), 0.0]
    p.cam_up[:] = [*map(float, u / focal), 0.0]
    p.volume_bounds[:] = list(dims)
    p.frame = int(frame)
    p.screen_size[:] = list(res)
    p.camera_jitter[:] = list(jitter)
    return p


def make_params(oracle, ao, light):
    p = oracle.Params()
    p.ao_samples = ao
    p.ambient_intensity = 0.6
    p.light_dir[:] = [float(np.float32(x)) for x in _unit(light)]
    p.light_intensity = 1.1
    p.light_color[:] = [1.0, 0.9, 0.8, 1.0]
    p.max_steps, p.ao_steps, p.max_bounces, p.shadows = 512, 64, 5, 1        # the shader's constants
    return p


LIGHT_UP, LIGHT_DOWN = (0.35, 0.8, -0.45), (-0.5, -0.3, 0.62)                 # the second one shines from below the horizon

# name: (position, viewing direction, ao samples, frame, jitter, light)
GEOMETRY_CASES = {
    "outside_ao4": ((19.3, 11.2, -21.0), (0.03, 0.02, 1.0), 4, 0, (0.3, -0.2), LIGHT_UP),
    "inside_ao1": ((30.4, 9.3, 6.6), (-0.8, 0.05, 0.6), 1, 31, (-0.45, 0.1), LIGHT_DOWN),
    "outside_ao0": ((-14.0, 15.5, -9.0), (0.9, -0.12, 0.55), 0, 32, (0.25, 0.4), LIGHT_UP),
    "inside_ao4": ((12.6, 6.4, 4.3), (0.55, 0.08, 0.83), 4, 2 ** 32 - 1, (0.1, -0.35), LIGHT_DOWN),
}


def geometry_case(oracle, name):
    pos, look, ao, frame, jitter, light = GEOMETRY_CASES[name]
    return make_push(oracle, DIMS, (W, H), pos, look, frame, jitter), make_params(oracle, ao, light)


def push_bytes(push):
    return np.frombuffer(bytes(push), np.uint8).copy()


def push_of(oracle, raw):
    return oracle.Push.from_buffer_copy(np.asarray(raw, np.uint8).tobytes())


def params_vector(p):
    return np.array([p.ao_samples, p.ambient_intensity, *p.light_dir, p.light_intensity, *p.light_color], np.float64)


def params_of(oracle, v):
    p = oracle.Params()
    p.ao_samples = int(v[0]); p.ambient_intensity = float(v[1])
    p.light_dir[:] = [float(x) for x in v[2:5]]; p.light_intensity = float(v[5]); p.light_color[:] = [float(x) for x in v[6:10]]
    p.max_steps, p.ao_steps, p.max_bounces, p.shadows = 512, 64, 5, 1
    return p


def ray_table(oracle, push):
    """(H, W, 3) primary directions by the oracle's vo_primary_ray."""
    w, h = push.screen_size[0], push.screen_size[1]
    return np.array([[oracle.primary_ray(push, x, y)[1] for x in range(w)] for y in range(h)], np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return bits(a) == bits(b)


def canonical_zero(a):
    """-0 -> +0: the one thing about the normal that no output of the pipeline can show (its only consumers are SNORM8 and sums)."""
    return np.asarray(a, np.float32) + np.float32(0.0)


# ---- denoiser --------------------------------------------------------------------------------------------------------------------

DENOISE_SIZES = ((37, 21), (72, 44))


def denoise_inputs(w, h):
    """colour RGBA8, normal RGBA8_SNORM, position RGBA32F (finite): noise, flat regions, hard edges; the frame border included."""
    rng = np.random.default_rng(w * 1000 + h)
    color = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    color[h // 4: h // 2, w // 5: w // 2] = (200, 40, 90, 0)                  # flat block, hard edges
    color[:, : w // 8] = (color[:, : w // 8] // 64) * 64                      # coarse steps up to the left border
    color[-3:, :] = (10, 250, 128, 0)                                         # flat up to the bottom border
    axes = np.array([(127, 0, 0, 0), (0, 127, 0, 0), (0, 0, -127, 0), (0, -127, 0, 0), (0, 0, 0, 0)], np.int8)
    normal = axes[rng.integers(0, 5, (h, w))]
    normal[h // 4: h // 2, w // 5: w // 2] = (0, 127, 0, 0)
    normal[0, :] = (-128, 0, 0, 0)                                            # the SNORM code that decodes through the clamp
    position = (rng.random((h, w, 4)).astype(np.float32) * np.float32(0.2)).astype(np.float32)
    position[..., 0] += np.linspace(0, 3, w, dtype=np.float32)[None, :]
    position[h // 4: h // 2, w // 5: w // 2] = (1.5, 2.0, 0.25, 0.0)
    position[..., 3] = 0.0
    position[h // 2:, w // 2:] = 0.0                                          # "sky"
    return color, normal, position


# ---- blit: the size pairs of test_gpu_temporal.test_blit_bit_exact, and its source image ---------------------------------------------

BLIT_SIZES = ((96, 54, 96, 54), (113, 63, 192, 108), (64, 36, 192, 108), (192, 108, 96, 54), (160, 90, 120, 120), (90, 160, 200, 100),
              (1, 1, 33, 17), (37, 5, 3, 29))


def blit_source(sw, sh, th):
    rng = np.random.default_rng(sw * 131 + th)
    img = rng.integers(0, 256, size=(sh, sw, 4), dtype=np.uint8)
    img[sh // 3: sh // 2, sw // 4: sw // 2] = (255, 0, 255, 255)
    img[0, :] = 0
    img[:, -1] = 255
    return img


# ---- the two documented divergences ------------------------------------------------------------------------------------------------

FACE_RES, AXIS_RES = (40, 28), (9, 7)


def face_case(oracle):
    """9.4-A: the solid z = 0 face of face_scene() from outside, no zero direction component."""
    return (make_push(oracle, (16, 12, 10), FACE_RES, (7.3, 5.6, -9.0), (0.04, 0.03, 1.0), 5, (0.0, 0.0)),
            make_params(oracle, 1, LIGHT_UP))


def axis_case(oracle):
    """9.4-I: scene() along +z from a lattice-free position, odd frame, no jitter: the centre column has dir.x == 0, the centre row
    dir.y == 0 (the basis is exact: right = (-1, 0, 0) / 2, up = (0, 1, 0) / 2)."""
    return (make_push(oracle, DIMS, AXIS_RES, (19.4, 6.3, -20.0), (0.0, 0.0, 1.0), 1, (0.0, 0.0), focal=2.0),
            make_params(oracle, 1, LIGHT_UP))


# ---- what the frames contain (not bit-critical: statistics for the non-triviality assertions) ---------------------------------------

def chain_stats(oracle, osn, push, par, metallic):
    """Per pixel: hit (bool), chain (-1 miss, 0 no bounce, k = rays of the bounce loop), end ('sky', 'plain', 'metal', ''), shadowed."""
    w, h = push.screen_size[0], push.screen_size[1]
    f = np.float32
    hit, chain, shadowed, end = np.zeros((h, w), bool), np.full((h, w), -1), np.zeros((h, w), bool), np.full((h, w), "", object)
    light = np.array(list(par.light_dir), f)
    for y in range(h):
        for x in range(w):
            s, d = oracle.primary_ray(push, x, y)
            r = oracle.trace_ray(osn, s, d)
            if r.material == 0:
                continue
            hit[y, x], chain[y, x] = True, 0
            p, n = np.array(list(r.pos), f), np.array(list(r.normal), f)
            shadowed[y, x] = oracle.trace_ray(osn, p + n * f(0.01), light).material != 0
            m = r.material
            while metallic[m] > 0 and chain[y, x] < 5:
                d = (d - f(2) * np.dot(n, d) * n).astype(f)
                r = oracle.trace_ray(osn, p + n * f(0.01), d)
                chain[y, x] += 1
                m = r.material
                if m == 0:
                    end[y, x] = "sky"
                    break
                p, n = np.array(list(r.pos), f), np.array(list(r.normal), f)
                end[y, x] = "metal" if metallic[m] > 0 else "plain"
    return hit, chain, end, shadowed
