"""The numeric spec's primitives (csrc/vrt_spec.h: sqrt_spec, div_spec, normalize3, atan2_spec, asin_spec, exp_spec, unorm8, snorm8,
wrap_texel) compiled for the HOST, held to the oracle's vo_spec_batch input by input: the link "host header == oracle" of the chain
DESIGN.md section 3 states.  The inputs are tests/spec_common.py's, the same the device is held to in tests/test_gpu_spec.py; of the
sweep over all 2^32 patterns of the one-argument primitives this file runs slices 0, 8, 15, 16, 24 and 31 (both signs' denormals and
zeros, the binades around 1 and 0.5, infinities and NaNs), and all 32 with VRT_SPEC_SWEEP=full.  Equality is of bit patterns; two
NaNs are equal whatever they carry, and the number of such pairs is printed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import spec_common as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "spec_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libspec_host.so")
HDR = os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_spec.h")
NT = 8
SWEEP = tuple(range(sp.SLICES)) if os.environ.get("VRT_SPEC_SWEEP", "") == "full" else sp.DEFAULT_SLICES
U32 = np.uint32
_cache = {}


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in (SRC, HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-pthread", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    l.spec_host_batch.restype = C.c_int
    l.spec_host_batch.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int]

    def run(fn, a, b=None, c=None):
        arrs = [None if x is None else np.ascontiguousarray(x, U32) for x in (a, b, c)]
        out = np.empty(arrs[0].size * sp.WORDS[fn], U32)
        rc = l.spec_host_batch(fn, *[None if x is None else x.ctypes.data for x in arrs], arrs[0].size, out.ctypes.data, NT)
        assert rc == 0, (fn, rc)
        return out
    return run


def _hold(host, oracle, fn, cls, what):
    a, b, c = cls
    exp = oracle.spec_batch(fn, a, b, c, nthreads=NT)
    sp.hold(host(fn, a, b, c), exp, fn, cls, what)
    return exp


def test_the_edge_set_holds_what_it_names():
    e = set(sp.edge_set().tolist())
    for v in (0x00000000, 0x80000000, 0x00000001, 0x007fffff, 0x00800000, 0x3f800000, 0x3f800001, 0x3f7fffff, 0x7f7fffff, 0xff7fffff,
              0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001, 0xffffffff, 0x3f000000, 0x3effffff, 0x3f000001):
        assert v in e, hex(v)
    assert sp.AIMED_COUNT == 7340032 and sp.WRAP_COUNT_AIMED == 1225 and sp.edge_set_prime().size == 176
    assert sorted(set(sp.DEFAULT_SLICES)) == [0, 8, 15, 16, 24, 31] and sp.SLICES << sp.SLICE_BITS == 1 << 32


def test_the_batch_is_the_oracles_own_functions(oracle):
    """vo_spec_batch adds no formula: on E it returns what the exported scalar functions return, one call at a time."""
    lib = oracle.lib()
    e = sp.edge_set()
    # (a signalling NaN cannot be handed to a scalar function from Python: the conversion to a Python float quiets it)
    e = e[~(sp.is_nan(e) & ((e & U32(0x00400000)) == 0))]
    assert e.size == 4096 - 6
    f = e.view(np.float32)
    scalar = {sp.FN_ASIN: lib.vo_asinf, sp.FN_EXP: lib.vo_expf, sp.FN_UNORM8: lib.vo_unorm8, sp.FN_SNORM8: lib.vo_snorm8}
    for fn, call in scalar.items():
        if fn in sp.FLOAT_OUT:
            exp = np.array([call(C.c_float(float(x))) for x in f], np.float32).view(U32)
        else:
            exp = np.array([call(C.c_float(float(x))) for x in f], np.int64).astype(np.int32).view(U32)
        assert sp.differences(oracle.spec_batch(fn, e, nthreads=3), exp, fn)[0].size == 0, sp.FN_NAMES[fn]
    y, x = e[::7][:500], e[::5][:500]
    exp = np.array([lib.vo_atan2f(C.c_float(float(a)), C.c_float(float(b))) for a, b in zip(y.view(np.float32), x.view(np.float32))], np.float32).view(U32)
    assert sp.differences(oracle.spec_batch(sp.FN_ATAN2, y, x, nthreads=2), exp, sp.FN_ATAN2)[0].size == 0
    with np.errstate(all="ignore"):
        assert sp.differences(oracle.spec_batch(sp.FN_SQRT, e), np.sqrt(f).view(U32), sp.FN_SQRT)[0].size == 0
        assert sp.differences(oracle.spec_batch(sp.FN_DIV, y, x), (y.view(np.float32) / x.view(np.float32)).view(U32), sp.FN_DIV)[0].size == 0
    # any number of threads gives the same words, and a fn or an array that is missing is refused
    assert all(np.array_equal(oracle.spec_batch(sp.FN_ASIN, e, nthreads=t), oracle.spec_batch(sp.FN_ASIN, e, nthreads=1)) for t in (2, 5, 16))
    for bad in (lambda: oracle.spec_batch(9, e), lambda: oracle.spec_batch(-1, e), lambda: oracle.spec_batch(sp.FN_DIV, e),
                lambda: oracle.spec_batch(sp.FN_NORMALIZE3, e, e)):
        with pytest.raises(ValueError):
            bad()
    assert oracle.spec_batch(sp.FN_EXP, np.zeros(0, U32)).size == 0


@pytest.mark.parametrize("half", (0, 1))
@pytest.mark.parametrize("k", SWEEP)
@pytest.mark.parametrize("fn", sp.ONE_ARG, ids=[sp.FN_NAMES[f] for f in sp.ONE_ARG])
def test_one_argument_slice(host, oracle, fn, k, half):
    """(Two cases a slice: where x * x underflows -- exp over |x| < 2^-63 -- a CPU takes seconds for 2^27 patterns.)"""
    _hold(host, oracle, fn, sp.slice_host(k, half), f"host {sp.FN_NAMES[fn]}, slice {k}, half {half}")


@pytest.mark.parametrize("fn", (sp.FN_DIV, sp.FN_ATAN2), ids=["div", "atan2"])
def test_pairs(host, oracle, fn):
    _hold(host, oracle, fn, sp.pairs_edges(), f"host {sp.FN_NAMES[fn]}, E x E")
    _hold(host, oracle, fn, sp.pairs_random(10 + fn), f"host {sp.FN_NAMES[fn]}, random pairs")


def _aimed(host, oracle):
    if "aimed" not in _cache:
        cls = sp.atan2_with_extras()
        exp = _hold(host, oracle, sp.FN_ATAN2, cls, "host atan2, aimed pairs")
        red = sp.atan2_is_red(cls[0], cls[1])
        for x in cls[:2] + (exp, red):
            x.setflags(write=False)
        _cache["aimed"] = cls, exp, red
    return _cache["aimed"]


def test_atan2_aimed_pairs_sit_on_both_sides(host, oracle):
    (y, x, _), exp, red = _aimed(host, oracle)
    n = sp.AIMED_COUNT
    assert not red[n] and not red[n + 1] and sp.is_nan(exp[n]) and exp[n + 1] == 0
    # the threshold group has lanes on either side of `red`; the swap group has |y| > |x|, == and <
    share = red[:n].mean()
    assert 0.5 < share < 0.9, share
    ay, ax = y[:n] & U32(0x7fffffff), x[:n] & U32(0x7fffffff)
    assert (ay > ax).sum() > n // 8 and (ay == ax).sum() > n // 20 and (ay < ax).sum() > n // 8
    a, b = sp.arrangement_sorted(red), sp.arrangement_mixed(red)
    sp.check_arrangements(red, a, b, sp.arrangement_single(red, 0, 4096))
    for name, idx in (("sorted", a), ("mixed", b)):
        sp.hold(host(sp.FN_ATAN2, y[idx], x[idx]), exp[idx], sp.FN_ATAN2, (y[idx], x[idx]), f"host atan2, aimed pairs, {name}")


@pytest.mark.parametrize("quarter", range(4))
def test_atan2_one_red_lane_per_wave(host, oracle, quarter):
    (y, x, _), exp, red = _aimed(host, oracle)
    waves = sp.arrangement_single_waves(red)
    w0, w1 = waves * quarter // 4, waves * (quarter + 1) // 4
    seen = np.zeros(sp.AIMED_COUNT + 2, bool)
    for c0 in range(w0, w1, 1 << 18):
        idx = sp.arrangement_single(red, c0, min(w1, c0 + (1 << 18)))
        seen[idx] = True
        sp.hold(host(sp.FN_ATAN2, y[idx], x[idx]), exp[idx], sp.FN_ATAN2, (y[idx], x[idx]), f"host atan2, one red lane a wave, waves {c0}..")
    assert seen[np.flatnonzero(red)[w0:w1]].all() and seen[-2:].all()


def test_normalize_edge_and_random_triples(host, oracle):
    _hold(host, oracle, sp.FN_NORMALIZE3, sp.triples_edges(), "host normalize3, E' x E' x E'")
    _hold(host, oracle, sp.FN_NORMALIZE3, sp.triples_random(21), "host normalize3, random triples")


@pytest.mark.parametrize("which,negative,position", sp.ONE_AXIS_CLASSES)
def test_normalize_one_axis(host, oracle, which, negative, position):
    cls = sp.triples_one_axis(which, negative, position)
    what = f"host normalize3, one axis {which} {'-' if negative else '+'} at {position}"
    _hold(host, oracle, sp.FN_NORMALIZE3, cls, what)
    x = cls[position]
    sp.hold_one_axis(host(sp.FN_NORMALIZE3, *cls), x, position, what)
    if position == 0:
        sq = sp.squares(x)
        root = _hold(host, oracle, sp.FN_SQRT, (sq, None, None), what + ", sqrt(x * x)")
        assert (root == (x & U32(0x7fffffff))).all(), what


def test_one_axis_identity_fails_outside_its_range(oracle):
    """hold_one_axis is a check: just below the range x * x is subnormal and loses bits, above it x * x overflows."""
    for x in (np.float32(float.fromhex("0x1.fffffep-70")), np.float32(float.fromhex("0x1p64"))):
        xs = np.asarray([x], np.float32).view(U32)
        z = np.zeros(1, U32)
        out = oracle.spec_batch(sp.FN_NORMALIZE3, xs, z, z)
        with pytest.raises(AssertionError):
            sp.hold_one_axis(out, xs, 0, "outside")


def test_wrap_texel(host, oracle):
    _hold(host, oracle, sp.FN_WRAP, sp.wrap_edges(), "host wrap_texel, E")
    u, n, _ = cls = sp.wrap_aimed()
    exp = _hold(host, oracle, sp.FN_WRAP, cls, "host wrap_texel, around k / n")
    assert (exp < n).all() and len(set(exp[n == 37].tolist())) >= 4


def test_the_rule_of_equality():
    a = np.asarray([0x3f800000, 0x7fc00000, 0x00000000, 0xffffff81], U32)
    assert sp.differences(a, a.copy(), sp.FN_ASIN)[0].size == 0
    b = a.copy(); b[1] = 0xffc00001                     # another NaN: equal, counted
    bad, payload = sp.differences(a, b, sp.FN_ASIN)
    assert bad.size == 0 and payload == 1
    b = a.copy(); b[2] = 0x80000000                     # the sign of zero
    assert sp.differences(a, b, sp.FN_ASIN)[0].tolist() == [2]
    b = a.copy(); b[3] = 0xffffff82                     # integers get no NaN rule: snorm8's -127 against -126
    assert sp.differences(a, b, sp.FN_SNORM8)[0].tolist() == [3]
    b = a.copy(); b[1] = 0x7f800000                     # NaN against inf
    assert sp.differences(a, b, sp.FN_ASIN)[0].tolist() == [1]
    with pytest.raises(AssertionError):
        sp.hold(a, b, sp.FN_ASIN, (a, None, None), "rule")
    with pytest.raises(AssertionError):
        sp.counted((a[:3], None, None), 4)
