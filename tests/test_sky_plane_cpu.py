"""When a launch uses a miss-colour plane: the host rule of csrc/vrt_miss_plane.h (sky_plane_key, sky_plane_select), compiled for
the CPU without HIP (tests/native/sky_plane_host.cpp) and driven through ctypes -- and once more as a stand-alone program built
with -fsanitize=address,undefined, whose main() runs its own script of launches over the same functions.

  * frames are grouped by the BYTES of their key: equal floats with different bit patterns (+0.0 / -0.0) are different views;
  * a one-ulp change in any of the thirteen ray-generation constants, another W or H, another fast_screen_div, a bumped sky
    generation each give a new key, and so a group of their own;
  * a group below the minimum gets no plane unless the context holds its plane already;
  * the context holds four planes: the fifth view evicts the one used longest ago, and no group of a launch evicts a plane that
    another group of the same launch uses;
  * sky_plane = 0 and launches that are not eligible select nothing and leave the cache alone."""
import ctypes as C
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "sky_plane_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libsky_plane_host.so")
SAN = os.path.join(ROOT, "tests", "native", "sky_plane_host_san")
HDR = os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_miss_plane.h")


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(p) for p in (SRC, HDR))


@pytest.fixture(scope="module")
def host():
    if _stale(LIB):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    for name in ("sp_planes", "sp_min_group", "sp_key_words"):
        getattr(l, name).restype = C.c_int32
    l.sp_key.argtypes = [C.POINTER(C.c_uint32), C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.POINTER(C.c_uint32)]
    l.sp_cache_new.restype = C.c_void_p
    l.sp_cache_free.argtypes = [C.c_void_p]
    l.sp_cache_clear.argtypes = [C.c_void_p]
    l.sp_cache_held.restype = C.c_int32
    l.sp_cache_held.argtypes = [C.c_void_p]
    l.sp_select.restype = C.c_int32
    l.sp_select.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32), C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
    return l


def _bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


# a plausible frame: cd, planeV, jx, jy, W, H, then cam_right -- as bit patterns
BASE = [_bits(v) for v in (0.0, 0.0, 1.0, 0.0, 0.5625, 0.0, 0.0, 0.0, 104.0, 40.0, 1.0, 0.0, 0.0)]


def key_of(host, consts=BASE, W=104, H=40, div=1, gen=5):
    out = (C.c_uint32 * host.sp_key_words())()
    host.sp_key((C.c_uint32 * 13)(*consts), W, H, div, gen, out)
    return tuple(out)


class Ctx:
    def __init__(self, host):
        self.h, self.c = host, host.sp_cache_new()

    def close(self):
        self.h.sp_cache_free(self.c)

    def launch(self, keys, enabled=1, eligible=1, min_group=None):
        n, kw = len(keys), self.h.sp_key_words()
        flat = (C.c_uint32 * max(1, n * kw))(*[w for k in keys for w in k])
        plane_of = (C.c_uint8 * max(1, n))()
        build = (C.c_int32 * self.h.sp_planes())()
        used = self.h.sp_select(self.c, enabled, eligible, n, flat, self.h.sp_min_group() if min_group is None else min_group, plane_of, build)
        return list(plane_of)[:n], list(build), used

    def held(self):
        return self.h.sp_cache_held(self.c)


@pytest.fixture()
def ctx(host):
    c = Ctx(host)
    yield c
    c.close()


def test_the_constants_of_the_rule(host):
    assert host.sp_planes() == 4
    assert 2 <= host.sp_min_group() <= 6          # low single digits (the 6 + 6 frame launch of the GPU test gets two planes)
    assert host.sp_key_words() == 18


def test_every_input_is_in_the_key_bit_for_bit(host):
    k0 = key_of(host)
    assert key_of(host) == k0
    seen = {k0}
    for i in range(13):                            # one ulp in each constant
        c = list(BASE)
        c[i] += 1
        k = key_of(host, consts=c)
        assert k not in seen, i
        seen.add(k)
    for kw in ({"W": 96}, {"H": 24}, {"W": 40, "H": 104}, {"div": 0}, {"gen": 6}, {"gen": 5 + (1 << 32)}):
        k = key_of(host, **kw)
        assert k not in seen, kw
        seen.add(k)
    # bitwise, not numeric: -0.0 == +0.0 as floats, another view as bytes
    c = list(BASE)
    c[0] = _bits(-0.0)
    assert key_of(host, consts=c) not in seen


def test_frames_are_grouped_by_key_and_small_groups_go_without(host, ctx):
    G = host.sp_min_group()
    a, b = key_of(host), key_of(host, gen=6)
    one_ulp = list(BASE)
    one_ulp[4] += 1
    d = key_of(host, consts=one_ulp)
    keys = [a, b] * G + [d] * (G - 1)              # two interleaved groups of G, one of G - 1
    plane_of, build, used = ctx.launch(keys)
    pa, pb = plane_of[0], plane_of[1]
    assert pa and pb and pa != pb and used == 2
    assert plane_of[:2 * G] == [pa, pb] * G
    assert plane_of[2 * G:] == [0] * (G - 1)
    assert build[pa - 1] == 0 and build[pb - 1] == 1 and sorted(build)[:2] == [-1, -1]
    assert ctx.held() == 2
    # the same launch again: both held, nothing built; and now ONE frame of a held view uses its plane
    plane_of2, build2, _ = ctx.launch(keys)
    assert plane_of2 == plane_of and build2 == [-1] * 4
    plane_of3, build3, used3 = ctx.launch([b])
    assert plane_of3 == [pb] and build3 == [-1] * 4 and used3 == 1
    # ... while one frame of a view nobody holds goes without, at G - 1 frames too, and gets one at G
    assert ctx.launch([d])[0] == [0]
    assert ctx.launch([d] * (G - 1))[0] == [0] * (G - 1)
    plane_of4, build4, _ = ctx.launch([d] * G)
    assert plane_of4[0] not in (0, pa, pb) and build4[plane_of4[0] - 1] == 0


def test_the_fifth_view_evicts_the_one_used_longest_ago(host, ctx):
    G = host.sp_min_group()
    views = [key_of(host, gen=10 + v) for v in range(5)]
    slots = []
    for v in range(4):
        plane_of, build, _ = ctx.launch([views[v]] * G)
        slots.append(plane_of[0])
    assert sorted(slots) == [1, 2, 3, 4] and ctx.held() == 4
    ctx.launch([views[0]])                         # view 0 is used again: view 1 is now the oldest
    plane_of, build, _ = ctx.launch([views[4]] * G)
    assert plane_of[0] == slots[1] and build[slots[1] - 1] == 0 and ctx.held() == 4
    assert ctx.launch([views[1]])[0] == [0]        # gone
    for v in (0, 2, 3, 4):
        assert ctx.launch([views[v]])[0] != [0], v


def test_a_launch_never_evicts_a_plane_it_uses(host, ctx):
    G = host.sp_min_group()
    views = [key_of(host, gen=20 + v) for v in range(6)]
    for v in range(4):
        ctx.launch([views[v]] * G)
    # views 0 .. 3 are held; a launch of views 0, 1, 2 (one frame each: held) and 4, 5 (G frames each: new) has one slot to give
    keys = [views[0], views[1], views[2]] + [views[4]] * G + [views[5]] * G
    plane_of, build, used = ctx.launch(keys)
    assert 0 not in plane_of[:3] and len(set(plane_of[:3])) == 3
    assert plane_of[3] not in (0,) + tuple(plane_of[:3]) and plane_of[3:3 + G] == [plane_of[3]] * G
    assert plane_of[3 + G:] == [0] * G and used == 4
    assert sum(1 for b in build if b >= 0) == 1 and build[plane_of[3] - 1] == 3


def test_off_and_not_eligible_select_nothing_and_keep_the_cache(host, ctx):
    G = host.sp_min_group()
    a, b = key_of(host), key_of(host, gen=9)
    ctx.launch([a] * G)
    assert ctx.held() == 1
    for enabled, eligible in ((0, 1), (1, 0), (0, 0)):
        plane_of, build, used = ctx.launch([a] * G + [b] * G, enabled=enabled, eligible=eligible)
        assert plane_of == [0] * (2 * G) and build == [-1] * 4 and used == 0
        assert ctx.held() == 1
    assert ctx.launch([a])[0] != [0]               # still there
    host.sp_cache_clear(ctx.c)
    assert ctx.held() == 0 and ctx.launch([a])[0] == [0]


def test_the_rule_under_address_and_undefined_behaviour_sanitizers():
    if _stale(SAN):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-DSKY_PLANE_MAIN", "-o", SAN, SRC])
    r = subprocess.run([SAN], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
    assert r.returncode == 0, r.stdout
    assert "sky_plane_host: ok" in r.stdout
