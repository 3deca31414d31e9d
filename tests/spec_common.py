"""What tests/test_spec_cpu.py (the host compile of csrc/vrt_spec.h) and tests/test_gpu_spec.py (vrt_debug_spec on the device) share:
the inputs on which a primitive of the numeric spec is held to the oracle's vo_spec_batch, and the rule of equality.

Everything is a uint32 bit pattern.  A CLASS of inputs is (a, b, c) -- arrays of equal length, b and c None where the primitive
does not read them -- and comes with the count it must have: a class that lost inputs fails its test (`counted`).

  E            4096 values: 256 exponents x 2 signs x the mantissas MANTISSAS (+-0, smallest / largest denormal, smallest normal,
               1 +- ulp, FLT_MAX, +-inf, signalling and quiet NaNs)
  one argument every bit pattern, in SLICES slices of 2^27 (slice k: k << 27 .. ((k + 1) << 27) - 1)
  pairs        E x E, 2^24 seeded random pairs; for atan2 also the aimed pairs (either side of the `red` threshold tan(pi/8) and of
               the `swap` boundary |y| == |x|) in three arrangements over the waves of 64 lanes
  triples      E' x E' x E', the one-axis triples of one_axis_len_ok's range, 2^22 seeded random triples
  wrap_texel   E and coordinates a few ulps around k / n, shifted by whole numbers, for seven texture sizes

E' is E at the eleven exponents E_PRIME_EXPONENTS (where x * x underflows, overflows, or is 0, 1, inf or NaN): 176 values, 176^3
triples."""
import numpy as np

FN_SQRT, FN_DIV, FN_ATAN2, FN_ASIN, FN_EXP, FN_UNORM8, FN_SNORM8, FN_WRAP, FN_NORMALIZE3 = range(9)
FN_NAMES = ("sqrt", "div", "atan2", "asin", "exp", "unorm8", "snorm8", "wrap_texel", "normalize3")
ONE_ARG = (FN_SQRT, FN_ASIN, FN_EXP, FN_UNORM8, FN_SNORM8)
FLOAT_OUT = (FN_SQRT, FN_DIV, FN_ATAN2, FN_ASIN, FN_EXP, FN_NORMALIZE3)      # the others answer integers: no NaN rule for them
NEEDS = {FN_SQRT: 1, FN_DIV: 2, FN_ATAN2: 2, FN_ASIN: 1, FN_EXP: 1, FN_UNORM8: 1, FN_SNORM8: 1, FN_WRAP: 2, FN_NORMALIZE3: 3}
WORDS = {fn: (3 if fn == FN_NORMALIZE3 else 1) for fn in range(9)}

MANTISSAS = (0, 1, 2, 0x3fffff, 0x400000, 0x400001, 0x7ffffe, 0x7fffff)
SLICE_BITS, SLICES = 27, 32
DEFAULT_SLICES = (0, 8, 15, 16, 24, 31)         # the CPU test's share of the sweep unless VRT_SPEC_SWEEP=full
WAVE = 64

U32 = np.uint32
_ABS, _INF = U32(0x7fffffff), U32(0x7f800000)


def counted(arrays, n):
    """The class with its count asserted: no input is skipped."""
    arrays = tuple(arrays)
    assert all(x is None or (x.dtype == U32 and x.ndim == 1 and x.size == n) for x in arrays) and arrays[0] is not None, \
        ([None if x is None else x.size for x in arrays], n)
    return arrays


def _values(exponents):
    e = np.asarray(list(exponents), U32)
    m = np.asarray(MANTISSAS, U32)
    s = np.asarray([0, 1], U32)
    return ((s[:, None, None] << U32(31)) | (e[None, :, None] << U32(23)) | m[None, None, :]).ravel()


def edge_set():
    e = _values(range(256))
    assert e.size == 4096 and np.unique(e).size == 4096
    return e


E_PRIME_EXPONENTS = (0, 1, 63, 64, 126, 127, 128, 190, 191, 254, 255)


def edge_set_prime():
    e = _values(E_PRIME_EXPONENTS)
    assert e.size == 176 and np.unique(e).size == 176
    return e


def is_nan(u):
    return (u & _ABS) > _INF


# ---- the rule of equality ---------------------------------------------------------------------------------------------------------

def differences(got, exp, fn):
    """(indices of the elements that differ, number of NaN pairs whose payloads or signs differ).  Bit patterns must be equal, the
    sign of zero included; two NaNs are equal whatever they carry (float-valued primitives only)."""
    got, exp = np.asarray(got, U32).ravel(), np.asarray(exp, U32).ravel()
    assert got.size == exp.size, (got.size, exp.size)
    if np.array_equal(got, exp):
        return np.zeros(0, np.int64), 0
    ne = got != exp
    if fn not in FLOAT_OUT:
        return np.flatnonzero(ne), 0
    both = is_nan(got)
    both &= is_nan(exp)
    both &= ne
    payload = int(np.count_nonzero(both))
    ne &= ~both
    return np.flatnonzero(ne), payload


def hold(got, exp, fn, inputs, what):
    """Asserts the rule; the message names the first elements that differ with their inputs.  Returns the payload count."""
    bad, payload = differences(got, exp, fn)
    if bad.size:
        w = WORDS[fn]
        first = [tuple(f"{int(x[i // w]):#010x}" for x in inputs if x is not None) + (f"got {int(np.asarray(got).ravel()[i]):#010x}",
                 f"oracle {int(np.asarray(exp).ravel()[i]):#010x}") for i in bad[:6]]
        raise AssertionError(f"{what}: {bad.size} of {np.asarray(exp).size} words differ from the oracle's {FN_NAMES[fn]}; first: {first}")
    print(f"{what}: {np.asarray(exp).size} words equal; NaN pairs with different payloads: {payload}")
    return payload


# ---- one argument -------------------------------------------------------------------------------------------------------------------

_base = {}


def slice_host(k, half=None):
    """Every bit pattern of slice k, ascending; half = 0 / 1: its lower / upper 2^26 (the CPU test runs a slice as two cases)."""
    assert 0 <= k < SLICES
    if "a" not in _base:
        _base["a"] = np.arange(1 << SLICE_BITS, dtype=U32)
        _base["a"].setflags(write=False)
    a = _base["a"] | U32(k << SLICE_BITS)
    if half is None:
        return counted((a, None, None), 1 << SLICE_BITS)
    h = 1 << (SLICE_BITS - 1)
    return counted((a[half * h:(half + 1) * h], None, None), h)


def slice_offset_i32(k):
    """k << 27 as the int32 a device tensor of int32 takes: torch.arange(2^27, int32) | offset are the slice's patterns."""
    v = k << SLICE_BITS
    return v - (1 << 32) if v >= 1 << 31 else v


# ---- pairs --------------------------------------------------------------------------------------------------------------------------

def pairs_edges():
    e = edge_set()
    a, b = np.repeat(e, e.size), np.tile(e, e.size)
    return counted((a, b, None), 4096 * 4096)


def pairs_random(seed):
    rng = np.random.default_rng(seed)
    n = 1 << 24
    return counted((rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32), rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32), None), n)


TAN_PI_8 = np.float32(0.4142135623730950)
AIMED_X, RED_ULPS, SWAP_ULPS = 1 << 16, tuple(range(-4, 5)), tuple(range(-2, 3))
AIMED_COUNT = AIMED_X * (len(RED_ULPS) + len(SWAP_ULPS)) * 4 * 2          # four sign combinations, and x and y exchanged


def _move(bits, j):
    """A non-negative float's pattern moved by j ulps, kept inside the non-negative patterns."""
    return np.clip(bits.astype(np.int64) + j, 0, 0x7fffffff).astype(U32)


def atan2_aimed(seed=2):
    """(y, x) patterns: for 2^16 positive x, 256 of each exponent with seeded mantissas, y = RN(x * tan(pi/8)f) moved by -4 .. +4
    ulps and y = x moved by -2 .. +2 ulps; each in the four sign combinations; each once more with x and y exchanged."""
    rng = np.random.default_rng(seed)
    x = ((np.arange(AIMED_X, dtype=U32) % U32(256)) << U32(23)) | rng.integers(0, 1 << 23, AIMED_X, dtype=np.uint64).astype(U32)
    with np.errstate(all="ignore"):
        yr = (x.view(np.float32) * TAN_PI_8).view(U32)
    ys = [_move(yr, j) for j in RED_ULPS] + [_move(x, j) for j in SWAP_ULPS]
    y = np.concatenate(ys)
    x = np.tile(x, len(ys))
    sy, sx = [], []
    for sgn_y in (0, 1):
        for sgn_x in (0, 1):
            sy.append(y | U32(sgn_y << 31)); sx.append(x | U32(sgn_x << 31))
    y, x = np.concatenate(sy), np.concatenate(sx)
    return counted((np.concatenate([y, x]), np.concatenate([x, y]), None), AIMED_COUNT)


def atan2_is_red(y, x):
    """Which pairs take atan_unit's reduction: t = smaller / larger > tan(pi/8)f, in IEEE float32 (what arranges the waves, never
    what a result is compared with).  NaN pairs and (0, 0) are not red."""
    ay, ax = (y & _ABS).view(np.float32), (x & _ABS).view(np.float32)
    with np.errstate(all="ignore"):
        swap = ay > ax
        t = np.where(swap, ax / ay, ay / ax)
        return t > TAN_PI_8


NAN_PAIR, ZERO_PAIR = (U32(0x7fc00000), U32(0x3f800000)), (U32(0), U32(0x80000000))         # atan2(NaN, 1) and atan2(+0, -0)


def atan2_with_extras(seed=2):
    """The aimed pairs followed by the two pairs arrangement (c) puts into every wave: element AIMED_COUNT is the NaN pair,
    AIMED_COUNT + 1 the (0, 0) pair."""
    y, x, _ = atan2_aimed(seed)
    y = np.concatenate([y, np.asarray([NAN_PAIR[0], ZERO_PAIR[0]], U32)])
    x = np.concatenate([x, np.asarray([NAN_PAIR[1], ZERO_PAIR[1]], U32)])
    return counted((y, x, None), AIMED_COUNT + 2)


def _pad_to_wave(idx):
    r = (-idx.size) % WAVE
    return np.concatenate([idx, np.resize(idx[-1:], r)]) if r else idx


def arrangement_sorted(red):
    """(a): indices into the aimed pairs such that every wave of 64 is all red or all not (groups padded with their last element)."""
    r, o = np.flatnonzero(red[:AIMED_COUNT]), np.flatnonzero(~red[:AIMED_COUNT])
    return np.concatenate([_pad_to_wave(r), _pad_to_wave(o)]).astype(np.int32)


def arrangement_mixed(red):
    """(b): red and not red alternate lane by lane, the shorter list repeated: every wave holds 32 of each."""
    r, o = np.flatnonzero(red[:AIMED_COUNT]), np.flatnonzero(~red[:AIMED_COUNT])
    n = max(r.size, o.size)
    n += (-n) % (WAVE // 2)
    idx = np.empty(2 * n, np.int32)
    idx[0::2] = np.resize(r, n)
    idx[1::2] = np.resize(o, n)
    return idx


def arrangement_single_waves(red):
    """(c) needs one wave per red pair."""
    return int(np.count_nonzero(red[:AIMED_COUNT]))


def arrangement_single(red, w0, w1):
    """(c), waves w0 .. w1 - 1: wave w holds the w-th red pair in lane w % 64, the NaN pair in lane (w + 21) % 64, the (0, 0) pair
    in lane (w + 42) % 64 and 61 pairs that are not red in the others (taken in order, 61 a wave, wrapping around)."""
    r, o = np.flatnonzero(red[:AIMED_COUNT]), np.flatnonzero(~red[:AIMED_COUNT])
    w = np.arange(w0, w1, dtype=np.int64)
    idx = np.empty((w.size, WAVE), np.int32)
    lane = np.arange(WAVE, dtype=np.int64)[None, :]
    l_red, l_nan, l_zero = (w % WAVE)[:, None], ((w + 21) % WAVE)[:, None], ((w + 42) % WAVE)[:, None]
    # the rank of a lane among the 61 others of its wave
    special = (lane == l_red) | (lane == l_nan) | (lane == l_zero)
    rank = np.cumsum(~special, axis=1) - 1
    idx[:] = o[(w[:, None] * 61 + rank) % o.size]
    rows = np.arange(w.size)
    idx[rows, l_red[:, 0]] = r[w]
    idx[rows, l_nan[:, 0]] = AIMED_COUNT
    idx[rows, l_zero[:, 0]] = AIMED_COUNT + 1
    return idx.ravel()


def check_arrangements(red, a, b, c_chunk):
    """The arrangements are what they claim: used by both tests before anything is submitted."""
    n = AIMED_COUNT
    full = np.append(red[:n], [False, False])
    ra = full[a].reshape(-1, WAVE).sum(1)
    assert ((ra == 0) | (ra == WAVE)).all() and np.unique(a).size == n
    rb = full[b].reshape(-1, WAVE).sum(1)
    assert (rb == WAVE // 2).all() and np.unique(b).size == n
    cc = c_chunk.reshape(-1, WAVE)
    assert (full[cc].sum(1) == 1).all() and ((cc == n).sum(1) == 1).all() and ((cc == n + 1).sum(1) == 1).all()


# ---- triples ------------------------------------------------------------------------------------------------------------------------

def triples_edges():
    e = edge_set_prime()
    n = e.size
    a = np.repeat(e, n * n)
    b = np.tile(np.repeat(e, n), n)
    c = np.tile(e, n * n)
    return counted((a, b, c), 176 ** 3)


def triples_random(seed):
    rng = np.random.default_rng(seed)
    n = 1 << 22
    return counted(tuple(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(U32) for _ in range(3)), n)


ONE_AXIS_ENDS = (127 - 60, 127 + 60)             # the exponent fields of 2^-60 and 2^60: VRT_ONE_AXIS_MIN / _MAX
ONE_AXIS_BETWEEN = tuple(range(127 - 59, 127 + 60))
ONE_AXIS_RANDOM = 1 << 16


def one_axis_values(which, negative, seed=4):
    """The x of a one-axis class: an end's exponent with EVERY mantissa, or ("between") the edge mantissas at every exponent between
    the ends and 2^16 seeded values there."""
    if which == "between":
        rng = np.random.default_rng(seed)
        e = rng.integers(ONE_AXIS_BETWEEN[0], ONE_AXIS_BETWEEN[-1] + 1, ONE_AXIS_RANDOM, dtype=np.uint64).astype(U32)
        x = np.concatenate([_values(ONE_AXIS_BETWEEN)[: len(ONE_AXIS_BETWEEN) * len(MANTISSAS)],
                            (e << U32(23)) | rng.integers(0, 1 << 23, ONE_AXIS_RANDOM, dtype=np.uint64).astype(U32)])
        n = len(ONE_AXIS_BETWEEN) * len(MANTISSAS) + ONE_AXIS_RANDOM
    else:
        assert which in ONE_AXIS_ENDS
        x = U32(which << 23) | np.arange(1 << 23, dtype=U32)
        n = 1 << 23
    x = x | U32((1 if negative else 0) << 31)
    return counted((x,), n)[0]


ONE_AXIS_CLASSES = [(w, neg, pos) for w in ONE_AXIS_ENDS + ("between",) for neg in (False, True) for pos in (0, 1, 2)]


def triples_one_axis(which, negative, position):
    """(x, 0, 0) with x in place `position`; the zeros are +0."""
    x = one_axis_values(which, negative)
    z = np.zeros_like(x)
    t = [z, z, z]
    t[position] = x
    return counted(t, x.size)


def hold_one_axis(out, x, position, what):
    """Besides equality with the oracle: len == |x| in one_axis_len_ok's range, i.e. the quotient x / len is exactly +-1 and the other
    two components are 0 / len = +0."""
    out = np.asarray(out, U32).reshape(-1, 3)
    one = (x & U32(0x80000000)) | U32(0x3f800000)
    assert (out[:, position] == one).all(), (what, "x / len3 is not +-1: len3 != |x|", int((out[:, position] != one).sum()))
    others = [p for p in range(3) if p != position]
    assert (out[:, others] == 0).all(), what


def squares(x):
    """RN(x * x) in IEEE float32: what len3 of a one-axis vector takes the root of (+0 +0 changes nothing)."""
    f = (x & _ABS).view(np.float32)
    return (f * f).view(U32)


# ---- wrap_texel -------------------------------------------------------------------------------------------------------------------

WRAP_SIZES = (1, 2, 37, 512, 4096, 8192, 1 << 20)
WRAP_SHIFTS = (-3, -1, 0, 1, 1000)
WRAP_COUNT_EDGES = len(WRAP_SIZES) * 4096
WRAP_COUNT_AIMED = len(WRAP_SIZES) * 5 * 7 * len(WRAP_SHIFTS)


def _step(bits, j):
    """Any finite float's pattern moved by j ulps along the number line (through zero: -denormal .. -0 / +0 .. +denormal)."""
    b = bits.astype(np.int64)
    key = np.where(b & 0x80000000, -(b & 0x7fffffff), b)
    key = key + j
    return np.where(key < 0, (-key) | 0x80000000, key).astype(U32)


def wrap_edges():
    e = edge_set()
    u = np.tile(e, len(WRAP_SIZES))
    n = np.repeat(np.asarray(WRAP_SIZES, U32), e.size)
    return counted((u, n, None), WRAP_COUNT_EDGES)


def wrap_aimed():
    us, ns = [], []
    for n in WRAP_SIZES:
        for k in (0, 1, n // 2, n - 1, n):
            base = np.asarray([np.float32(k) / np.float32(n)], np.float32).view(U32)
            for j in range(-3, 4):
                u = _step(base, j).view(np.float32)
                for s in WRAP_SHIFTS:
                    us.append((u + np.float32(s)).view(U32)[0]); ns.append(n)
    return counted((np.asarray(us, U32), np.asarray(ns, U32), None), WRAP_COUNT_AIMED)


# ---- the sky texel from the oracle's primitives -----------------------------------------------------------------------------------

def oracle_sky_texels(oracle, dirs, w, h, nthreads=8):
    """Column 0 of vrt_debug_sky_texels from vo_spec_batch: normalize, atan2(d.z, d.x), asin(-d.y), the shader's two multiply-adds in
    float32 (voxel_volume.frag:101: each product and each sum rounded once), wrap_texel; x | y << 16."""
    v = np.ascontiguousarray(dirs, np.float32).view(U32).reshape(-1, 3)
    n = v.shape[0]
    d = oracle.spec_batch(FN_NORMALIZE3, v[:, 0].copy(), v[:, 1].copy(), v[:, 2].copy(), nthreads=nthreads)
    at = oracle.spec_batch(FN_ATAN2, d[:, 2].copy(), d[:, 0].copy(), nthreads=nthreads).view(np.float32)
    an = oracle.spec_batch(FN_ASIN, d[:, 1] ^ U32(0x80000000), nthreads=nthreads).view(np.float32)
    with np.errstate(all="ignore"):
        u = (at * np.float32(0.1591)).astype(np.float32) + np.float32(0.5)
        t = (an * np.float32(0.3183)).astype(np.float32) + np.float32(0.5)
    sx = oracle.spec_batch(FN_WRAP, u.view(U32), np.full(n, w, U32), nthreads=nthreads)
    sy = oracle.spec_batch(FN_WRAP, t.view(U32), np.full(n, h, U32), nthreads=nthreads)
    return sx | (sy << U32(16))
