"""csrc/vrt_brush.h without a device: the header compiled with g++ (tests/native/brush_host.cpp) against the restatement in
Python integers (tests/brush_reference.py) -- exhaustively on small volumes, at the extremes of the parameter ranges, the 48
orientations --, a program of its own under ASan + UBSan (tests/native/brush_fuzz.cpp), and the C-ABI surface of
vrt_scene_brush / vrt_scene_stamp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import brush_native as N
import brush_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "tests", "native", "brush_fuzz.cpp")

DIMS = (37, 29, 40)                                 # W, H, D

# (shape, p): centres on voxel centres (odd) and on corners (even); semi-axes 1, 2, 3 and unequal; capsules along an axis,
# diagonal and with a == b; boxes inside, across a face and around the volume
SHAPES = [
    (R.ELLIPSOID, (21, 15, 33, 1, 1, 1)), (R.ELLIPSOID, (20, 14, 32, 1, 1, 1)), (R.ELLIPSOID, (21, 14, 33, 1, 1, 1)),
    (R.ELLIPSOID, (21, 15, 33, 2, 2, 2)), (R.ELLIPSOID, (20, 14, 32, 2, 2, 2)), (R.ELLIPSOID, (21, 15, 33, 3, 3, 3)), (R.ELLIPSOID, (20, 16, 32, 3, 3, 3)),
    (R.ELLIPSOID, (31, 21, 41, 9, 4, 13)), (R.ELLIPSOID, (30, 22, 40, 1, 7, 2)), (R.ELLIPSOID, (40, 30, 39, 16, 15, 3)), (R.ELLIPSOID, (37, 29, 41, 23, 23, 23)),
    (R.ELLIPSOID, (1, 1, 1, 5, 6, 7)), (R.ELLIPSOID, (74, 58, 80, 9, 9, 9)), (R.ELLIPSOID, (-6, 20, 20, 8, 3, 3)), (R.ELLIPSOID, (37, 29, 40, 200, 100, 150)),
    (R.CAPSULE, (11, 15, 21, 51, 15, 21, 5)), (R.CAPSULE, (20, 9, 30, 20, 49, 30, 4)), (R.CAPSULE, (31, 31, 9, 31, 31, 70, 1)),
    (R.CAPSULE, (9, 9, 9, 61, 45, 71, 6)), (R.CAPSULE, (60, 8, 70, 10, 50, 12, 3)), (R.CAPSULE, (30, 30, 30, 30, 30, 30, 7)), (R.CAPSULE, (31, 29, 33, 31, 29, 33, 1)),
    (R.CAPSULE, (-20, -10, 5, 90, 70, 60, 9)), (R.CAPSULE, (30, 30, 30, 31, 30, 30, 2)), (R.CAPSULE, (-4096, 20, 20, 12288, 30, 40, 5)),
    (R.BOX, (5, 6, 7, 9, 4, 11)), (R.BOX, (-3, 10, 36, 8, 30, 9)), (R.BOX, (-5, -5, -5, 60, 60, 60)), (R.BOX, (36, 28, 39, 1, 1, 1)), (R.BOX, (0, 0, 0, 1, 1, 1)),
]
MODES = [(R.SET, 9, 0), (R.SET, 0, 0), (R.PAINT, 9, 0), (R.ADD, 9, 0), (R.REPLACE, 9, 40), (R.REPLACE, 0, 40), (R.REPLACE, 9, 0)]


def volume(seed=1):
    W, H, D = DIMS
    rng = np.random.default_rng(seed)
    vol = ((rng.random((D, H, W)) < 0.35) * rng.integers(1, 60, (D, H, W))).astype(np.uint8)
    vol[12:22, 5:20, 8:30] = 40
    return vol


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_header_covers_what_python_integers_cover(k):
    """every voxel of the volume: brush_inside (which answers outside its bounds without a product) equals the bare inequality"""
    shape, p = SHAPES[k]
    assert R.shape_ok(shape, p) and N.shape_ok(shape, p)
    exp = R.inside_mask(shape, p, DIMS, everywhere=True)
    got = N.mask(shape, p, DIMS)
    assert (got == exp).all(), (shape, p, np.argwhere(got != exp)[:4])
    assert (R.inside_mask(shape, p, DIMS) == exp).all()                     # the reference's own shortcut loses nothing
    lo, hi = R.bounds(shape, p)
    assert N.bounds(shape, p) == (lo, hi)
    assert N.clip(lo, hi, DIMS) == R.clip(lo, hi, DIMS)
    if exp.any():                                                           # the bounds hold every covered voxel ...
        zs, ys, xs = np.nonzero(exp)
        c = R.clip(lo, hi, DIMS)
        assert c is not None
        for v, a in ((xs, 0), (ys, 1), (zs, 2)):
            assert c[0][a] <= v.min() and v.max() < c[0][a] + c[1][a]


def test_known_shapes():
    one = R.inside_mask(R.ELLIPSOID, (21, 15, 33, 1, 1, 1), DIMS, everywhere=True)
    assert one.sum() == 1 and one[16, 7, 10]                                # r = (1, 1, 1) on a voxel's centre: that voxel
    assert R.inside_mask(R.ELLIPSOID, (20, 14, 32, 1, 1, 1), DIMS, everywhere=True).sum() == 0      # on a corner: the eight centres lie sqrt(3) away
    assert R.inside_mask(R.ELLIPSOID, (20, 14, 32, 2, 2, 2), DIMS, everywhere=True).sum() == 8
    assert R.inside_mask(R.ELLIPSOID, (21, 15, 33, 2, 2, 2), DIMS, everywhere=True).sum() == 7      # the voxel and its six face neighbours
    s = R.inside_mask(R.ELLIPSOID, (21, 15, 33, 3, 3, 3), DIMS, everywhere=True)
    c = R.inside_mask(R.CAPSULE, (21, 15, 33, 21, 15, 33, 3), DIMS, everywhere=True)
    assert (s == c).all() and s.sum() == 19                                 # a == b is the sphere; |d|^2 <= 9 with even d: 1 + 6 + 12
    line = R.inside_mask(R.CAPSULE, (11, 15, 21, 51, 15, 21, 1), DIMS, everywhere=True)
    assert line.sum() == 21 and line[10, 7, 5:26].all()


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_every_shape_times_every_mode(k):
    shape, p = SHAPES[k]
    vol = volume(k)
    for mode, vid, match in MODES:
        exp, res = R.brush(vol, shape, mode, p, vid, match, everywhere=True)
        rc, got, gres = N.brush(vol, shape, mode, p, vid, match)
        assert rc == 0 and (got == exp).all() and gres == res, (shape, p, mode, vid, match, gres, res)
        inside = R.inside_mask(shape, p, DIMS)
        assert (exp[~inside] == vol[~inside]).all()
        if mode == R.PAINT:
            assert ((exp != 0) == (vol != 0)).all()
        if mode == R.ADD:
            assert (exp[vol != 0] == vol[vol != 0]).all()


def test_modes_value_by_value():
    for mode in (R.SET, R.PAINT, R.ADD, R.REPLACE):
        for old in (0, 1, 40, 255):
            for vid in (0, 1, 40, 255):
                for match in (0, 40):
                    if R.mode_ok(mode, vid, match):
                        assert N.value(mode, old, vid, match) == int(R.value(mode, np.array([old], np.uint8), vid, match)[0])
    for mode, vid, match, ok in ((R.SET, 0, 0, True), (R.PAINT, 0, 0, False), (R.ADD, 0, 9, False), (R.PAINT, 1, 1, True), (R.REPLACE, 5, 5, False),
                                 (R.REPLACE, 0, 5, True), (R.REPLACE, 5, 0, True), (4, 1, 0, False), (-1, 1, 0, False)):
        assert N.mode_ok(mode, vid, match) == ok == R.mode_ok(mode, vid, match)


def _bounds_points(lo, hi):
    """the voxels of the bounds' corners, edge and face centres and middle, and the same one voxel further out"""
    pts = []
    for g in (0, 1):
        for k in range(27):
            pts.append([(lo[a] - g, (lo[a] + hi[a] - 1) // 2, hi[a] - 1 + g)[(k // 3 ** a) % 3] for a in range(3)])
    return pts


def test_extreme_ellipsoids_equal_python_integers():
    """semi-axes of 1024 and 1023 / 1024 / 1 mixes: the largest products the header forms, at the bounds' corners and face centres"""
    rng = np.random.default_rng(3)
    cases = [(c, r) for r in ((1024, 1024, 1024), (1023, 1024, 1), (1, 1023, 1024), (1024, 1, 1023), (1023, 1023, 1023), (1024, 1024, 1), (1, 1, 1024))
             for c in ((4097, 4097, 4097), (4096, 4096, 4096), (0, 8191, 1), (-1024, 9216, 4095), (2 ** 31 - 1, -2 ** 31, 0))]
    n_in = 0
    for c, r in cases:
        p = tuple(c) + tuple(r)
        assert N.shape_ok(R.ELLIPSOID, p)
        lo, hi = R.bounds(R.ELLIPSOID, p)
        assert N.bounds(R.ELLIPSOID, p) == (lo, hi)
        pts = _bounds_points(lo, hi)
        # voxels next to the surface: along each axis the last voxel inside and the first outside, through the centre
        for a in range(3):
            for v in (lo[a], lo[a] + 1, hi[a] - 2, hi[a] - 1):
                q = [(lo[b] + hi[b] - 1) // 2 for b in range(3)]
                q[a] = v
                pts.append(q)
        pts += [[int(rng.integers(lo[a], hi[a])) for a in range(3)] for _ in range(200)]
        pts = [q for q in pts if all(-2 ** 31 <= v < 2 ** 31 for v in q)]
        exp = np.array([R.inside(R.ELLIPSOID, p, *q) for q in pts])
        # the terms really are as large as the header's comment says, and no larger
        big = max(abs((2 * q[a] + 1 - c[a])) for q in pts for a in range(3) if lo[a] <= q[a] < hi[a])
        assert big <= max(r)
        got = N.inside(R.ELLIPSOID, p, pts)
        assert (got == exp).all(), (p, [q for q, g, e in zip(pts, got, exp) if g != e][:3])
        n_in += int(exp.sum())
    assert n_in > 500
    assert 3 * (2 ** 10) ** 6 < 2 ** 63                                       # the bound of vrt_brush.h: three terms of at most 2^60


def test_extreme_capsules_equal_python_integers():
    """end points at -4096 and 12288, r = 1024: at voxels within r of the segment and at the bounds' corners"""
    rng = np.random.default_rng(4)
    E = (-4096, 12288)
    ends = [(a, b) for a in [(x, y, z) for x in E for y in E for z in E] for b in [(x, y, z) for x in E for y in E for z in E]]
    ends += [((-4096, 0, 12288), (-4095, 1, 12287)), ((100, 100, 100), (100, 100, 100)), ((12288, 12288, 12288), (12288, 12288, -4096))]
    worst = 0
    n_in = 0
    for a, b in ends:
        for r in (1024, 1023, 1):
            p = tuple(a) + tuple(b) + (r,)
            assert N.shape_ok(R.CAPSULE, p)
            lo, hi = R.bounds(R.CAPSULE, p)
            assert N.bounds(R.CAPSULE, p) == (lo, hi)
            pts = _bounds_points(lo, hi)
            for _ in range(40):
                t = int(rng.integers(0, 1025))
                at = [a[i] + (b[i] - a[i]) * t // 1024 + int(rng.integers(-r - 2, r + 3)) for i in range(3)]
                pts.append([v // 2 for v in at])
            exp = np.array([R.inside(R.CAPSULE, p, *q) for q in pts])
            got = N.inside(R.CAPSULE, p, pts)
            assert (got == exp).all(), (p, [q for q, g, e in zip(pts, got, exp) if g != e][:3])
            n_in += int(exp.sum())
            # the products of the header's comment, in Python integers, over the points that lie inside the bounds
            e = [b[i] - a[i] for i in range(3)]
            L2 = sum(v * v for v in e)
            for q in pts:
                if all(lo[i] <= q[i] < hi[i] for i in range(3)):
                    da = [2 * q[i] + 1 - a[i] for i in range(3)]
                    worst = max(worst, sum(v * v for v in da) * L2, sum(da[i] * e[i] for i in range(3)) ** 2, r * r * L2)
    assert n_in > 1000
    assert 2 ** 59 < worst < 2 ** 60 < 2 ** 63                               # the extremes are reached, and they fit


def test_ranges_are_refused_outside():
    ok = (0, 0, 0, 1, 1, 1, 1)
    for shape in (R.BOX, R.ELLIPSOID, R.CAPSULE):
        assert N.shape_ok(shape, ok) and R.shape_ok(shape, ok)
    for shape, i, vals in ((R.ELLIPSOID, 3, (0, -1, 1025)), (R.ELLIPSOID, 5, (0, 1025)), (R.CAPSULE, 6, (0, -3, 1025)), (R.CAPSULE, 0, (-4097, 12289)),
                           (R.CAPSULE, 5, (-4097, 12289)), (R.BOX, 4, (0, -1, 2 ** 30 + 1))):
        for v in vals:
            p = list(ok); p[i] = v
            assert not N.shape_ok(shape, p) and not R.shape_ok(shape, p), (shape, p)
    for shape, i, vals in ((R.ELLIPSOID, 3, (1, 1024)), (R.CAPSULE, 6, (1, 1024)), (R.CAPSULE, 0, (-4096, 12288)), (R.BOX, 4, (1, 2 ** 30)), (R.BOX, 0, (-2 ** 31, 2 ** 31 - 1)),
                           (R.ELLIPSOID, 0, (-2 ** 31, 2 ** 31 - 1))):
        for v in vals:
            p = list(ok); p[i] = v
            assert N.shape_ok(shape, p) and R.shape_ok(shape, p), (shape, p)
            assert N.bounds(shape, p) == R.bounds(shape, p)
    assert not N.shape_ok(3, ok) and not N.shape_ok(-1, ok)


def test_clipping():
    for lo, hi in (((-5, 3, 2), (4, 9, 50)), ((37, 0, 0), (40, 5, 5)), ((-9, -9, -9), (0, 5, 5)), ((0, 0, 0), (37, 29, 40)), ((36, 28, 39), (99, 99, 99)),
                   ((-2 ** 31, -2 ** 31, 5), (2 ** 31 + 2 ** 30, 1, 6)), ((10, 10, 10), (10, 12, 12))):
        assert N.clip(lo, hi, DIMS) == R.clip(lo, hi, DIMS), (lo, hi)
    assert R.clip((-9, -9, -9), (0, 5, 5), DIMS) is None and R.clip((-5, 3, 2), (4, 9, 50), DIMS) == ([0, 3, 2], [4, 6, 38])
    vol = volume()
    out, res = R.brush(vol, R.ELLIPSOID, R.SET, (-40, -40, -40, 9, 9, 9), 5)                 # wholly outside: nothing, and no error
    assert (out == vol).all() and res == (0, [0, 0, 0], [0, 0, 0])
    assert N.brush(vol, R.ELLIPSOID, R.SET, (-40, -40, -40, 9, 9, 9), 5)[2] == res
    out, res = R.brush(vol, R.ELLIPSOID, R.SET, (0, 0, 0, 7, 7, 7), 200)                     # a corner of the volume keeps an eighth
    assert 0 < res[0] < 40 and res[1] == [0, 0, 0]


def test_extent_check_at_its_edges():
    """brush_extent_ok, the check between an extent kernel's record and the edit made from it, against its restatement in Python
    integers: per axis (mn, mx, clo, csize) at each edge, the other two axes inside, so each axis in turn is the only failing one"""
    def ok(mn, mx, clo, cs):
        return all(mn[a] >= clo[a] and mx[a] >= mn[a] and mx[a] < clo[a] + cs[a] for a in range(3))

    I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
    edges = [                                                   # (mn, mx, clo, csize) of one axis, and what the check makes of it
        ((5, 11, 5, 7), True),                                  # mn == clo and mx == clo + csize - 1
        ((5, 12, 5, 7), False),                                 # mx == clo + csize
        ((4, 11, 5, 7), False),                                 # mn == clo - 1
        ((9, 8, 5, 7), False),                                  # mx == mn - 1
        ((I32_MAX, I32_MIN, 5, 7), False),                      # the record nothing touched
        ((4095, 4095, 4095, 1), True),                          # the top of the largest volume
        ((0, 2 ** 30 - 1, 0, 2 ** 30), True),                   # the 64-bit sum ...
        ((0, 2 ** 30, 0, 2 ** 30), False),
        ((I32_MAX, I32_MAX, I32_MAX, 1), True),                 # ... which a 32-bit one would wrap
        ((I32_MAX, I32_MAX, I32_MAX - 1, 1), False),
    ]
    inside = (6, 9, 5, 7)
    assert N.extent_ok(*([v] * 3 for v in inside)) and ok(*([v] * 3 for v in inside))
    for a in range(3):
        for edge, exp in edges:
            args = [[edge[i] if b == a else inside[i] for b in range(3)] for i in range(4)]
            assert ok(*args) == exp, (a, edge)
            assert N.extent_ok(*args) == exp, (a, edge)
    assert not N.extent_ok([I32_MAX] * 3, [I32_MIN] * 3, [0, 0, 0], [37, 29, 40])       # brush_record_init() on every axis


def test_orientations_are_the_48_symmetries():
    size = (5, 3, 2)                                                                         # asymmetric: no two orientations coincide
    src = np.arange(1, 31, dtype=np.uint8).reshape(2, 3, 5)                                  # [z, y, x], every voxel its own id
    assert len(R.ORIENTS) == 48 == len(set(R.ORIENTS)) and all(N.orient_ok(o) == R.orient_ok(o) for o in range(-0, 80))
    assert [o for o in range(80) if N.orient_ok(o)] == sorted(R.ORIENTS)
    images = set()
    for o in R.ORIENTS:
        ds = N.stamp_dst_size(o, size)
        assert ds == R.stamp_dst_size(o, size) and sorted(ds) == [2, 3, 5]
        img = np.zeros((ds[2], ds[1], ds[0]), np.uint8)
        for dz in range(ds[2]):
            for dy in range(ds[1]):
                for dx in range(ds[0]):
                    s = N.stamp_source(o, size, (dx, dy, dz))
                    assert s == R.stamp_source(o, size, (dx, dy, dz)) and all(0 <= s[a] < size[a] for a in range(3))
                    img[dz, dy, dx] = src[s[2], s[1], s[0]]
        assert sorted(img.ravel().tolist()) == list(range(1, 31))                           # a bijection onto stamp_dst_size
        assert (img == R.oriented(src, o)).all()                                            # the reference's transpose-and-flip is the same map
        images.add((tuple(ds), img.tobytes()))
    assert len(images) == 48                                                                # distinct
    assert (R.oriented(src, 0) == src).all() and N.stamp_source(0, size, (4, 1, 1)) == [4, 1, 1]
    assert N.stamp_source(1 << 3, size, (0, 1, 1)) == [4, 1, 1] and N.stamp_source(2, size, (1, 4, 0)) == [4, 1, 0]
    for old in (0, 7):
        for s in (0, 9):
            for skip in (False, True):
                assert N.stamp_value(old, s, skip) == (old if skip and s == 0 else s)


def test_stamp_reference():
    rng = np.random.default_rng(6)
    dst = rng.integers(0, 5, (12, 10, 14)).astype(np.uint8)
    src = rng.integers(0, 3, (9, 8, 11)).astype(np.uint8)
    out, res = R.stamp(dst, (2, 3, 4), src, (1, 2, 3), (5, 3, 2))
    assert (out[4:6, 3:6, 2:7] == src[3:5, 2:5, 1:6]).all() and res[0] == int((out != dst).sum())
    out, _ = R.stamp(dst, (2, 3, 4), src, (1, 2, 3), (5, 3, 2), skip_empty=True)
    part = src[3:5, 2:5, 1:6]
    assert (out[4:6, 3:6, 2:7] == np.where(part == 0, dst[4:6, 3:6, 2:7], part)).all()
    out, res = R.stamp(dst, (-3, 8, 11), src, (0, 0, 0), (5, 3, 2))                          # clipped at two faces
    assert (out[11:12, 8:10, 0:2] == src[0:1, 0:2, 3:5]).all()
    assert R.stamp(dst, (14, 0, 0), src, (0, 0, 0), (5, 3, 2))[1][0] == 0                    # wholly outside
    self_out, _ = R.stamp(dst, (3, 0, 0), dst, (0, 0, 0), (8, 10, 12))                       # overlapping: the old content is copied
    assert (self_out[:, :, 3:11] == dst[:, :, 0:8]).all()


def test_fuzz_program_under_asan_and_ubsan(tmp_path):
    """tests/native/brush_fuzz.cpp, a program of its own, with -fsanitize=address,undefined and no recovery: random and extreme
    parameters through every function of the header; signed overflow would end it"""
    exe = str(tmp_path / "brush_fuzz_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, FUZZ])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed, "4000"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        m = re.match(r"(\d+) predicates, (\d+) inside", r.stdout)
        assert m and int(m.group(1)) > 1_000_000 and int(m.group(2)) > 100_000, r.stdout


def _header():
    with open(os.path.join(ROOT, "include", "vrt.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_header_exports_and_binding(vrt):
    hdr = _header()
    for name in ("vrt_scene_brush", "vrt_scene_stamp"):
        assert re.search(r"\bint\s+%s\s*\(\s*struct\s+vrt_ctx\s*\*" % name, hdr), name           # spelled `struct vrt_ctx*`
        assert name in vrt._capi.SYMBOLS
        assert getattr(vrt.lib(), name) is not None                                          # exported by libvrt_hip.so
    for name, val in (("VRT_BRUSH_BOX", R.BOX), ("VRT_BRUSH_ELLIPSOID", R.ELLIPSOID), ("VRT_BRUSH_CAPSULE", R.CAPSULE), ("VRT_BRUSH_SET", R.SET),
                      ("VRT_BRUSH_PAINT", R.PAINT), ("VRT_BRUSH_ADD", R.ADD), ("VRT_BRUSH_REPLACE", R.REPLACE), ("VRT_STAMP_SKIP_EMPTY", R.SKIP_EMPTY)):
        m = re.search(r"#define\s+%s\s+(\d+)" % name, hdr)
        assert m and int(m.group(1)) == val, name
    K = vrt._capi
    assert C.sizeof(K.Brush) == 48 and C.sizeof(K.BrushResult) == 32
    assert (K.BRUSH_BOX, K.BRUSH_ELLIPSOID, K.BRUSH_CAPSULE) == (R.BOX, R.ELLIPSOID, R.CAPSULE)
    assert (K.BRUSH_SET, K.BRUSH_PAINT, K.BRUSH_ADD, K.BRUSH_REPLACE) == (R.SET, R.PAINT, R.ADD, R.REPLACE) and K.STAMP_SKIP_EMPTY == R.SKIP_EMPTY


def test_argument_errors_need_no_context(vrt):
    l, K = vrt.lib(), vrt._capi
    b = K.Brush(shape=R.ELLIPSOID, mode=R.SET, id=1)
    b.p[3:6] = [2, 2, 2]
    res = K.BrushResult()
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3
    fake = C.c_void_p(8)                                          # never dereferenced: the NULL argument is found first
    for args in ((None, fake, C.byref(b), C.byref(res)), (fake, None, C.byref(b), C.byref(res)), (fake, fake, None, C.byref(res))):
        assert l.vrt_scene_brush(*args) == 1 and "vrt_scene_brush" in l.vrt_last_error().decode()
    for args in ((None, fake, i3(), fake, i3(), u3(1, 1, 1)), (fake, None, i3(), fake, i3(), u3(1, 1, 1)), (fake, fake, None, fake, i3(), u3(1, 1, 1)),
                 (fake, fake, i3(), None, i3(), u3(1, 1, 1)), (fake, fake, i3(), fake, None, u3(1, 1, 1)), (fake, fake, i3(), fake, i3(), None)):
        assert l.vrt_scene_stamp(*args, 0, 0, C.byref(res)) == 1 and "vrt_scene_stamp" in l.vrt_last_error().decode()
