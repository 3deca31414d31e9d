"""The numeric spec's primitives on the DEVICE (vrt_debug_spec: one primitive of csrc/vrt_spec.h per element, bit patterns in and
out) held to the oracle's vo_spec_batch input by input -- the link "device == oracle" of the chain DESIGN.md section 3 states, on
chosen floats, where frames only show what a few cameras happen to produce.  The inputs are tests/spec_common.py's, the same the
host compile of the header is held to in tests/test_spec_cpu.py: every bit pattern of the one-argument primitives in 32 slices of
2^27; E x E, random and aimed pairs for atan2 and division, the aimed pairs in three arrangements over the waves (atan_unit's device
branch decides per wave whether it divides at all); edge, one-axis and random triples for normalize3; wrap_texel around k / n.
Equality is of bit patterns; two NaNs are equal whatever they carry, and the number of such pairs is printed.  The last test closes
fast == device spec == oracle: column 0 of vrt_debug_sky_texels against the texel computed from vo_spec_batch.

What this cannot show: the kernel pins the header under the library's flags in a unit of its own; the copies inlined into the render
and denoise kernels stay pinned by the frame tests."""
import ctypes as C

import numpy as np
import pytest

import spec_common as sp
import stream_common as sc
from test_gpu_sky import _directions, _noise_sky
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

NT = 16
U32 = np.uint32
P = C.c_void_p
_cache = {}


def _ptr(t):
    return P(t.data_ptr()) if t is not None else None


def _device(vrt, engine, fn, arrays, n, out=None):
    """vrt_debug_spec over device tensors (int32 views of the patterns) -> the output tensor, after the one synchronise."""
    import torch
    if out is None:
        out = torch.full((n * sp.WORDS[fn],), 0x5a5a5a5a, dtype=torch.int32, device=engine.torch_device)
    vrt._capi.check(vrt.lib().vrt_debug_spec(engine.ctx, fn, *[_ptr(t) for t in arrays], n, _ptr(out)))
    engine.synchronize()
    return out


def _up(engine, x):
    import torch
    return None if x is None else torch.from_numpy(np.array(x, copy=True).view(np.int32)).to(engine.torch_device)


def _hold(vrt, oracle, engine, fn, cls, what):
    exp = oracle.spec_batch(fn, *cls, nthreads=NT)
    got = _device(vrt, engine, fn, [_up(engine, x) for x in cls], cls[0].size).cpu().numpy().view(U32)
    sp.hold(got, exp, fn, cls, what)
    return exp, got


@pytest.fixture(scope="module")
def sweep(engine):
    """The 2^27 low words of a slice, made once on the device, and the slice's output buffer."""
    import torch
    base = torch.arange(1 << sp.SLICE_BITS, dtype=torch.int32, device=engine.torch_device)
    out = torch.empty(1 << sp.SLICE_BITS, dtype=torch.int32, device=engine.torch_device)
    yield base, out
    del base, out
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", range(sp.SLICES))
@pytest.mark.parametrize("fn", sp.ONE_ARG, ids=[sp.FN_NAMES[f] for f in sp.ONE_ARG])
def test_one_argument_slice(vrt, oracle, engine, sweep, fn, k):
    base, out = sweep
    a = base | sp.slice_offset_i32(k)
    assert a.numel() == 1 << sp.SLICE_BITS and int(a[0].item()) & 0xffffffff == k << sp.SLICE_BITS
    out.fill_(0x5a5a5a5a)
    got = _device(vrt, engine, fn, [a, None, None], a.numel(), out=out).cpu().numpy().view(U32)
    cls = sp.slice_host(k)
    sp.hold(got, oracle.spec_batch(fn, cls[0], nthreads=NT), fn, cls, f"device {sp.FN_NAMES[fn]}, slice {k}")


@pytest.mark.parametrize("fn", (sp.FN_DIV, sp.FN_ATAN2), ids=["div", "atan2"])
def test_pairs_of_edges(vrt, oracle, engine, fn):
    _hold(vrt, oracle, engine, fn, sp.pairs_edges(), f"device {sp.FN_NAMES[fn]}, E x E")


@pytest.mark.parametrize("fn", (sp.FN_DIV, sp.FN_ATAN2), ids=["div", "atan2"])
def test_pairs_at_random(vrt, oracle, engine, fn):
    _hold(vrt, oracle, engine, fn, sp.pairs_random(10 + fn), f"device {sp.FN_NAMES[fn]}, random pairs")


def _aimed(vrt, oracle, engine):
    """The aimed pairs and their two extras: the oracle's words (host and device copies) and which pairs are red, made once."""
    if "aimed" not in _cache:
        cls = sp.atan2_with_extras()
        exp = oracle.spec_batch(sp.FN_ATAN2, *cls, nthreads=NT)
        red = sp.atan2_is_red(cls[0], cls[1])
        for x in cls[:2] + (exp, red):
            x.setflags(write=False)
        _cache["aimed"] = cls, exp, red, _up(engine, cls[0]), _up(engine, cls[1]), _up(engine, exp)
    return _cache["aimed"]


def _arranged(vrt, engine, aimed, idx, what):
    """Submits the pairs in the order idx; every lane against the oracle's word of its pair, on the device (NaN rule as
    spec_common.differences).  Returns the device's words per PAIR (the last lane that held it) and which pairs were held."""
    import torch
    (y, x, _), exp, red, yd, xd, ed = aimed
    it = torch.from_numpy(idx).to(engine.torch_device).long()
    got = _device(vrt, engine, sp.FN_ATAN2, [yd[it].contiguous(), xd[it].contiguous(), None], it.numel())
    want = ed[it]
    nan = lambda t: (t & 0x7fffffff) > 0x7f800000
    ne = got != want
    both = ne & nan(got) & nan(want)
    bad = ne & ~both
    nbad = int(bad.sum().item())
    print(f"{what}: {it.numel()} lanes; NaN pairs with different payloads: {int(both.sum().item())}")
    if nbad:
        i = int(torch.nonzero(bad)[0].item()); j = int(idx[i])
        raise AssertionError(f"{what}: {nbad} lanes differ from the oracle's atan2; first: lane {i} (wave {i // 64}), y {int(y[j]):#010x}, "
                             f"x {int(x[j]):#010x}, got {int(got[i].item()) & 0xffffffff:#010x}, oracle {int(exp[j]):#010x}")
    per_pair = torch.zeros(sp.AIMED_COUNT + 2, dtype=torch.int32, device=engine.torch_device)
    held = torch.zeros(sp.AIMED_COUNT + 2, dtype=torch.bool, device=engine.torch_device)
    per_pair[it] = got
    held[it] = True
    # every lane that held a pair answered the same word for it (NaNs as one)
    again = per_pair[it]
    assert int(((again != got) & ~(nan(again) & nan(got))).sum().item()) == 0, what
    return per_pair, held


def test_atan2_aimed_pairs_in_whole_and_mixed_waves(vrt, oracle, engine):
    """(a) waves that are all red or all not, (b) waves of 32 and 32: the device against the oracle lane by lane, and (a) against
    (b) pair by pair."""
    import torch
    aimed = _aimed(vrt, oracle, engine)
    (y, x, _), exp, red = aimed[:3]
    a, b = sp.arrangement_sorted(red), sp.arrangement_mixed(red)
    sp.check_arrangements(red, a, b, sp.arrangement_single(red, 0, 4096))
    _hold(vrt, oracle, engine, sp.FN_ATAN2, (y, x, None), "device atan2, aimed pairs as generated")
    pa, ha = _arranged(vrt, engine, aimed, a, "device atan2, (a) uniform waves")
    pb, hb = _arranged(vrt, engine, aimed, b, "device atan2, (b) mixed waves")
    n = sp.AIMED_COUNT
    assert bool(ha[:n].all()) and bool(hb[:n].all())
    nan = lambda t: (t & 0x7fffffff) > 0x7f800000
    assert int(((pa[:n] != pb[:n]) & ~(nan(pa[:n]) & nan(pb[:n]))).sum().item()) == 0
    _cache["per_pair_a"] = pa


C_PARTS = 8


@pytest.mark.parametrize("part", range(C_PARTS))
def test_atan2_one_red_lane_per_wave(vrt, oracle, engine, part):
    """(c): every red pair alone among 61 that are not, a NaN lane and a (0, 0) lane -- against the oracle lane by lane, and against
    what arrangement (a) answered for the same pairs."""
    import torch
    aimed = _aimed(vrt, oracle, engine)
    red = aimed[2]
    if "per_pair_a" not in _cache:
        _cache["per_pair_a"] = _arranged(vrt, engine, aimed, sp.arrangement_sorted(red), "device atan2, (a) uniform waves")[0]
    waves = sp.arrangement_single_waves(red)
    w0, w1 = waves * part // C_PARTS, waves * (part + 1) // C_PARTS
    idx = sp.arrangement_single(red, w0, w1)
    assert idx.size == (w1 - w0) * sp.WAVE
    pc, hc = _arranged(vrt, engine, aimed, idx, f"device atan2, (c) one red lane a wave, waves {w0} .. {w1 - 1}")
    mine = torch.from_numpy(np.flatnonzero(red)[w0:w1]).to(engine.torch_device).long()
    assert bool(hc[mine].all()) and bool(hc[-2:].all())
    pa = _cache["per_pair_a"]
    nan = lambda t: (t & 0x7fffffff) > 0x7f800000
    differ = hc[:sp.AIMED_COUNT] & (pc[:sp.AIMED_COUNT] != pa[:sp.AIMED_COUNT]) & ~(nan(pc[:sp.AIMED_COUNT]) & nan(pa[:sp.AIMED_COUNT]))
    assert int(differ.sum().item()) == 0


def test_normalize_edge_triples(vrt, oracle, engine):
    _hold(vrt, oracle, engine, sp.FN_NORMALIZE3, sp.triples_edges(), "device normalize3, E' x E' x E'")


def test_normalize_random_triples(vrt, oracle, engine):
    _hold(vrt, oracle, engine, sp.FN_NORMALIZE3, sp.triples_random(21), "device normalize3, random triples")


@pytest.mark.parametrize("which,negative,position", sp.ONE_AXIS_CLASSES)
def test_normalize_one_axis(vrt, oracle, engine, which, negative, position):
    cls = sp.triples_one_axis(which, negative, position)
    what = f"device normalize3, one axis {which} {'-' if negative else '+'} at {position}"
    _, got = _hold(vrt, oracle, engine, sp.FN_NORMALIZE3, cls, what)
    x = cls[position]
    sp.hold_one_axis(got, x, position, what)
    if position == 0:
        _, root = _hold(vrt, oracle, engine, sp.FN_SQRT, (sp.squares(x), None, None), what + ", sqrt(x * x)")
        assert (root == (x & U32(0x7fffffff))).all(), what


def test_wrap_texel(vrt, oracle, engine):
    _hold(vrt, oracle, engine, sp.FN_WRAP, sp.wrap_edges(), "device wrap_texel, E")
    _hold(vrt, oracle, engine, sp.FN_WRAP, sp.wrap_aimed(), "device wrap_texel, around k / n")


def _small(fn):
    """One small class per primitive: 4099 elements (a last wave of three lanes) of E, combined with itself in other orders."""
    e = sp.edge_set()
    a, b, c = np.resize(e, 4099), np.resize(e[::-1][5:], 4099), np.resize(e[::3], 4099)
    if fn == sp.FN_WRAP:
        b = np.resize(np.asarray(sp.WRAP_SIZES, U32), 4099)
    return (a, b, c)[:sp.NEEDS[fn]]


@pytest.mark.parametrize("kind", sc.KINDS)
def test_every_primitive_on_the_three_kinds_of_stream(vrt, oracle, kind):
    """stream_common's kinds: the HIP null stream, the context's own non-blocking stream, a torch side stream -- the nine launches
    enqueued without a wait between them into poisoned outputs, one synchronise, then the oracle."""
    import torch
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        eng = vrt.Engine(0, use_torch_stream=kind != "own")
        try:
            classes = {fn: tuple(_small(fn)) + (None,) * (3 - sp.NEEDS[fn]) for fn in range(9)}
            dev = {fn: [_up(eng, x) for x in cls] for fn, cls in classes.items()}
            outs = {fn: torch.full(((4099 + 64) * sp.WORDS[fn] * 4,), sc.POISON, dtype=torch.uint8, device=eng.torch_device).view(torch.int32)
                    for fn in range(9)}
            torch.cuda.synchronize()
            for fn in range(9):
                vrt._capi.check(vrt.lib().vrt_debug_spec(eng.ctx, fn, *[_ptr(t) for t in dev[fn]], 4099, _ptr(outs[fn])))
            eng.synchronize()
            for fn in range(9):
                got = outs[fn].cpu().numpy().view(U32)
                w = 4099 * sp.WORDS[fn]
                assert (got[w:] == U32(sc.POISON * 0x01010101)).all(), (kind, sp.FN_NAMES[fn], "wrote past its n elements")
                sp.hold(got[:w], oracle.spec_batch(fn, *classes[fn], nthreads=4), fn, classes[fn], f"device {sp.FN_NAMES[fn]} on {kind}")
        finally:
            eng.destroy()


def test_errors_of_the_entry(vrt, engine):
    import torch
    lib, INVALID, UNSUPPORTED = vrt.lib(), 1, 7               # VRT_ERR_INVALID, VRT_ERR_UNSUPPORTED (include/vrt.h)
    a = torch.zeros(64, dtype=torch.int32, device=engine.torch_device)
    out = torch.full((192,), 7, dtype=torch.int32, device=engine.torch_device)
    p, o = _ptr(a), _ptr(out)
    assert lib.vrt_debug_spec(None, 0, p, None, None, 64, o) == INVALID
    assert lib.vrt_debug_spec(engine.ctx, 9, p, p, p, 64, o) == INVALID and b"unknown fn" in lib.vrt_last_error()
    assert lib.vrt_debug_spec(engine.ctx, 0xffffffff, p, p, p, 64, o) == INVALID
    for fn in range(9):
        assert lib.vrt_debug_spec(engine.ctx, fn, None, p, p, 64, o) == INVALID, fn
        assert lib.vrt_debug_spec(engine.ctx, fn, p, p, p, 64, None) == INVALID, fn
        assert (lib.vrt_debug_spec(engine.ctx, fn, p, None, p, 64, o) == INVALID) == (sp.NEEDS[fn] >= 2), fn
        assert (lib.vrt_debug_spec(engine.ctx, fn, p, p, None, 64, o) == INVALID) == (sp.NEEDS[fn] >= 3), fn
        assert lib.vrt_debug_spec(engine.ctx, fn, p, p, p, 0, o) == vrt._capi.VRT_OK, fn           # nothing to do
    assert lib.vrt_debug_spec(engine.ctx, 0, p, None, None, (1 << 31) + 1, o) == UNSUPPORTED
    engine.synchronize()
    # the refused calls and the empty ones wrote nothing; the arrays a primitive does not read may be NULL
    assert bool((out[64:] == 7).all())
    vrt._capi.check(lib.vrt_debug_spec(engine.ctx, sp.FN_EXP, p, None, None, 64, o))
    engine.synchronize()
    assert bool((out[:64] == 0x3f800000).all()) and bool((out[64:] == 7).all())                      # exp(+0) == 1


@pytest.mark.parametrize("w,h", [(512, 256), (37, 11), (1, 1), (8192, 16)])
def test_device_spec_texel_is_the_oracles(vrt, oracle, engine, w, h):
    """Column 0 of vrt_debug_sky_texels (normalize3, atan2_spec, asin_spec, the two multiply-adds, wrap_texel inlined into
    k_debug_sky) on the direction sets of tests/test_gpu_sky.py against the same texel from vo_spec_batch."""
    import torch
    n = 1 << 22
    vol = np.zeros((8, 8, 8), np.uint8); vol[4, 4, 4] = 1
    scene = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt), sky=_noise_sky(w, h, 1), noise=vrt.synthetic.blue_noise_standin(8))
    try:
        d = _directions(torch, engine.torch_device, w, h, n, 100)
        assert tuple(d.shape) == (n, 3)
        out = torch.zeros((n, 4), dtype=torch.int32, device=engine.torch_device)
        vrt._capi.check(vrt.lib().vrt_debug_sky_texels(engine.ctx, scene.handle, P(d.data_ptr()), n, P(out.data_ptr())))
        engine.synchronize()
        got = out[:, 0].contiguous().cpu().numpy().view(U32)
        dirs = d.cpu().numpy()
        exp = sp.oracle_sky_texels(oracle, dirs, w, h, nthreads=NT)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (bad.size, [(dirs[i].tolist(), hex(int(got[i])), hex(int(exp[i]))) for i in bad[:4]])
        assert len(np.unique(exp)) > min(w * h, 1000) // 2
    finally:
        scene.destroy()
