"""The rules around the kernels, past their first iteration (tests/launch_shapes_common.py has the tables and what numpy can say about
them, tests/test_launch_shapes_cpu.py proves the tables without a device):

  A. frame batches         the ninth slot (a table in device memory), the 257th frame (a second launch), the fifth table launch
                           without a synchronise (a ring slot used again)
  B. strip / halo copies   the 65th image (a second launch), per-image shards, packed buffers of different heights in one call
  C. segment lengths       k_denoise_pair and k_denoise_ver in segments longer than the minimum, for every tap offset, with a last
                           segment shorter than R; the segment count forced through "denoise_pair_wgs"
  D. tolerance kernels     k_denoise_fast at both tile heights and the FAST form of k_denoise_lds: "denoise_verified" = 0 with
                           VRT_DENOISE_FAST, the one mode no other test launches
  E. "tags_async"          = 2 takes the second stream at every launch, so the path can be held to "changes speed only"

Every frame, image and row is compared bit for bit with a single call, with numpy or with the oracle; outputs are pre-filled with a
poison byte so that a frame or row nobody wrote shows.  Where a defect could only show while the device is still busy with the
launches before (a ring slot or a tag buffer overwritten too early), the sequence is enqueued behind a few milliseconds of other
work on the stream (_stall): the host then runs ahead of the device by the whole sequence."""
import ctypes as C

import numpy as np
import pytest
import torch

import denoise_shard_common as dsc
import launch_shapes_common as lsc
from helpers import camera_push, compare_planes, metallic_palette

pytestmark = pytest.mark.gpu

P = C.c_void_p
SPEC = {"color8": (np.uint8, (4,)), "depth": (np.float32, ()), "motion": (np.float32, (2,)), "mask8": (np.uint8, ()),
        "position": (np.float32, (4,)), "normal8": (np.int8, (4,)), "hit_id": (np.uint8, ())}       # the six reference targets + hit_id
NAMES = list(SPEC)


class Planes:
    """The output planes of n frames, every frame its own, every byte pre-filled with the poison."""

    def __init__(self, vrt, dev, n, res):
        self.n, (self.W, self.H) = n, res
        self.t = {}
        for name, (dt, tail) in SPEC.items():
            nbytes = self.W * self.H * np.dtype(dt).itemsize * int(np.prod(tail, dtype=np.int64))
            self.t[name] = torch.full((n, nbytes), lsc.POISON, dtype=torch.uint8, device=dev)
        self.c = (vrt._capi.Frame * n)()
        for f in range(n):
            for name, t in self.t.items():
                setattr(self.c[f], name, t[f].data_ptr())

    def bytes(self):
        """name -> uint8 (n, H, bytes per row)"""
        return {name: t.cpu().numpy().reshape(self.n, self.H, -1) for name, t in self.t.items()}

    @staticmethod
    def typed(b, f):
        """frame f of bytes() as the arrays the oracle returns"""
        out = {}
        for name, (dt, tail) in SPEC.items():
            a = np.ascontiguousarray(b[name][f])
            out[name] = a.view(dt).reshape((a.shape[0], -1) + tail)
        return out


def _stall(dev):
    """A few milliseconds of work on torch's stream, which is the context's: what is enqueued next waits behind it."""
    x = torch.zeros(1 << 28, dtype=torch.float32, device=dev)
    for _ in range(16):
        x.add_(1.0)
    return x


def _same(got, exp, names, what):
    for name in names:
        bad = np.flatnonzero((got[name] != exp[name]).any(axis=tuple(range(1, got[name].ndim))))
        assert bad.size == 0, f"{what}: plane {name} differs in frames {bad[:8].tolist()} ({bad.size} in all)"


def _settings(vrt, res, which):
    st = vrt.VoxelRenderSettings.primary_only(res) if which == "primary_only" else vrt.VoxelRenderSettings(targetResolution=res)
    st.fsrSetttings.enable = False
    assert tuple(st.renderResolution()) == tuple(res)
    return st


def _single(vrt, engine, scene, stc, push, frame_c, shard=None):
    vrt._capi.check(vrt.lib().vrt_render_geometry(engine.ctx, scene.handle, C.byref(push), C.byref(stc), C.byref(frame_c),
                                                  C.byref(shard) if shard is not None else None))


# ---- A. batches past their first launch ---------------------------------------------------------------------------------------------

class _World:
    pass


@pytest.fixture(scope="module")
def world(vrt, oracle, engine):
    """One scene of 32^3 with metallic ids, the poses, and the single vrt_render_geometry call of every pose under both settings."""
    w = _World()
    rng = np.random.default_rng(31)
    vol = (rng.random(lsc.BATCH_DIMS) < 0.05).astype(np.uint8) * rng.integers(1, 256, lsc.BATCH_DIMS).astype(np.uint8)
    vol[10:22, 12:20, 10:22] = 210                                   # a metallic block in the middle
    pal = metallic_palette(vrt)
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    w.scene = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    w.oscene = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    w.n = max(lsc.BATCH_SIZES)
    w.pushes = [camera_push(vrt, lsc.BATCH_DIMS, lsc.BATCH_RES, **p) for p in lsc.poses(w.n)]
    w.st, w.singles, w.oracle = {}, {}, {}
    for which in ("primary_only", "default"):
        st = w.st[which] = _settings(vrt, lsc.BATCH_RES, which)
        stc = st.to_c()
        out = Planes(vrt, engine.torch_device, w.n, lsc.BATCH_RES)
        for f in range(w.n):
            _single(vrt, engine, w.scene, stc, w.pushes[f], out.c[f])
        engine.synchronize()
        w.singles[which] = out.bytes()
    hit = w.singles["default"]["hit_id"]
    assert (hit == 0).all((1, 2)).any() and (hit != 0).any((1, 2)).sum() > w.n // 2           # some frames look away, most do not
    assert len({hit[f].tobytes() for f in range(w.n)}) > w.n // 2                             # and the poses really differ

    def expected(which, f):
        if (which, f) not in w.oracle:
            w.oracle[(which, f)] = oracle.render(w.oscene, w.pushes[f], oracle.params_from(w.st[which].to_c()), planes=NAMES, nthreads=8)
        return w.oracle[(which, f)]
    w.expected = expected
    return w


@pytest.mark.parametrize("which", ["primary_only", "default"])
@pytest.mark.parametrize("n", lsc.BATCH_SIZES)
def test_batch_past_the_first_launch(vrt, engine, world, n, which):
    """vrt_render_geometry_batch of n frames: every frame equals the single call of its pose, six of them the oracle."""
    w = world
    out = Planes(vrt, engine.torch_device, n, lsc.BATCH_RES)
    stc = w.st[which].to_c()
    pushes = (vrt._capi.Push * n)(*w.pushes[:n])
    vrt._capi.check(vrt.lib().vrt_render_geometry_batch(engine.ctx, w.scene.handle, n, pushes, C.byref(stc), out.c, None))
    engine.synchronize()
    got = out.bytes()
    _same(got, {k: v[:n] for k, v in w.singles[which].items()}, NAMES, f"batch of {n}, {which}")
    for f in sorted({f for f in lsc.ORACLE_FRAMES + (n - 1,) if f < n}):
        bad = compare_planes(Planes.typed(got, f), w.expected(which, f), NAMES)
        assert not bad, (n, which, f, bad)


def test_slots_past_the_first_launch(vrt, engine, world):
    """vrt_render_geometry_slots, 260 frames, frame f with the strips of rank f % 3 of a 3-rank, 16-row split of 40 rows: own rows
    equal the single sharded call, every other row still holds the poison."""
    w = world
    n, res, N, S = lsc.SLOTS_N, lsc.SLOTS_RES, lsc.SLOTS_RANKS, lsc.SLOTS_STRIP
    stc = _settings(vrt, res, "default").to_c()
    pushes = (vrt._capi.Push * n)(*[camera_push(vrt, lsc.BATCH_DIMS, res, **p) for p in lsc.poses(n)])
    shards = (vrt._capi.Shard * n)(*[vrt._capi.Shard(f % N, N, S) for f in range(n)])
    single, out = Planes(vrt, engine.torch_device, n, res), Planes(vrt, engine.torch_device, n, res)
    for f in range(n):
        _single(vrt, engine, w.scene, stc, pushes[f], single.c[f], shards[f])
    vrt._capi.check(vrt.lib().vrt_render_geometry_slots(engine.ctx, w.scene.handle, n, pushes, C.byref(stc), out.c, shards))
    engine.synchronize()
    got, exp = out.bytes(), single.bytes()
    own = np.zeros((n, res[1]), bool)
    for f in range(n):
        own[f, dsc.owned_rows(res[1], f % N, N, S)] = True
    assert own.any(1).all() and not own.all(1).any()
    for name in NAMES:
        g, e = got[name], exp[name]
        assert (e[~own] == lsc.POISON).all(), name                                   # (the single calls wrote their own rows only, too)
        bad = np.flatnonzero(((g != e) & own[:, :, None]).any((1, 2)))
        assert bad.size == 0, f"plane {name}: own rows differ from the single call in frames {bad[:8].tolist()}"
        bad = np.flatnonzero(((g != lsc.POISON) & ~own[:, :, None]).any((1, 2)))
        assert bad.size == 0, f"plane {name}: rows of another rank written in frames {bad[:8].tolist()}"
    assert (exp["mask8"][own] != lsc.POISON).any()


def test_table_ring_is_reused_without_a_synchronise(vrt, engine, world):
    """Six table launches of nine frames on one context, enqueued behind a busy stream and synchronised once at the end: the fifth
    takes the ring slot of the first.  Every launch its own poses and outputs; every frame equals its single call."""
    w = world
    L, n, which = lsc.RING_LAUNCHES, lsc.RING_N, "default"
    stc = w.st[which].to_c()
    outs = [Planes(vrt, engine.torch_device, n, lsc.BATCH_RES) for _ in range(L)]
    pushes = [(vrt._capi.Push * n)(*w.pushes[k * n:(k + 1) * n]) for k in range(L)]
    engine.synchronize()
    keep = _stall(engine.torch_device)
    for k in range(L):
        vrt._capi.check(vrt.lib().vrt_render_geometry_batch(engine.ctx, w.scene.handle, n, pushes[k], C.byref(stc), outs[k].c, None))
    engine.synchronize()
    del keep
    for k in range(L):
        _same(outs[k].bytes(), {m: v[k * n:(k + 1) * n] for m, v in w.singles[which].items()}, NAMES, f"table launch {k}")


# ---- B. strip and halo copies past 64 images ------------------------------------------------------------------------------------

GUARD_ROWS, FILL = 2, 77


class _Packed:
    """n packed buffers side by side in one allocation: slot i holds rows[i] rows that belong to image i, then rows up to the largest
    buffer of the call plus GUARD_ROWS that belong to nobody.  A copy that runs past an image's own buffer lands in rows that are
    inside the allocation and are looked at afterwards."""

    def __init__(self, dev, rows, row_bytes, fill=None):
        self.rows, self.slot = list(rows), max(rows) + GUARD_ROWS
        host = np.full((len(rows), self.slot, row_bytes), FILL, np.uint8)
        if fill is not None:
            for i, a in enumerate(fill):
                host[i, :len(a)] = a
        self.host, self.t = host, torch.from_numpy(host).to(dev)

    def ptrs(self):
        return (P * len(self.rows))(*[self.t[i].data_ptr() for i in range(len(self.rows))])

    def check(self, want, maps, what):
        got = self.t.cpu().numpy()
        for i, (m, wnt) in enumerate(zip(maps, want)):
            ok = m >= 0
            assert (got[i, :len(m)][ok] == wnt[ok]).all(), f"{what}: image {i}, packed rows differ"
            assert np.isin(got[i, :len(m)][~ok], (0, FILL)).all(), f"{what}: image {i}, a padding row holds image bytes"
            assert (got[i, len(m):] == FILL).all(), f"{what}: image {i}, written past the end of its packed buffer"


def _copies(vrt, engine, n, bpp, shards, rng, null_at=None):
    """All four batch copies over n images with the given (rank, nranks) per image, against the numpy row maps."""
    D, L, ctx, dev = vrt.distributed, vrt.lib(), engine.ctx, engine.torch_device
    W, H, S, halo = lsc.COPY_W, lsc.COPY_H, lsc.COPY_STRIP, lsc.COPY_HALO
    rb = W * bpp
    check = vrt._capi.check
    fulls = rng.integers(0, 256, (n, H, rb), dtype=np.uint8)
    dfull = torch.from_numpy(fulls).to(dev)
    full_ptrs = (P * n)(*[dfull[i].data_ptr() for i in range(n)])
    cs = (vrt._capi.Shard * n)(*[vrt._capi.Shard(r, N, S) for r, N in shards])

    def unpack_into_poison(fn, packed, maps, *tail):
        poison = rng.integers(0, 256, (n, H, rb), dtype=np.uint8)
        dst = torch.from_numpy(poison).to(dev)
        ptrs = (P * n)(*[dst[i].data_ptr() for i in range(n)])
        check(fn(ctx, n, packed.ptrs(), ptrs, W, H, bpp, cs, *tail))
        engine.synchronize()
        want = poison.copy()
        for i in range(n):
            D.unpack_np(packed.host[i, :len(maps[i])], want[i], maps[i])
        bad = np.flatnonzero((dst.cpu().numpy() != want).any((1, 2)))
        assert bad.size == 0, f"{fn.__name__}: images {bad[:8].tolist()} differ (only mapped rows may change)"
        return ptrs, dst, poison

    # own rows: pack with ONE shard for all images (the frames of a batch on a rank), unpack with one per image (the root of a gather)
    r1, N1 = shards[1]
    one = vrt._capi.Shard(r1, N1, S)
    m1 = lsc.own_row_map(H, r1, N1, S, D)
    packed = _Packed(dev, [len(m1)] * n, rb)
    check(L.vrt_pack_rows_batch(ctx, n, full_ptrs, packed.ptrs(), W, H, bpp, C.byref(one)))
    engine.synchronize()
    packed.check([D.pack_np(fulls[i], m1) for i in range(n)], [m1] * n, "vrt_pack_rows_batch")
    maps = [lsc.own_row_map(H, r, N, S, D) for r, N in shards]
    packed = _Packed(dev, [len(m) for m in maps], rb, fill=[D.pack_np(fulls[i], maps[i]) for i in range(n)])
    unpack_into_poison(L.vrt_unpack_rows_batch, packed, maps)
    # halo rows, both directions
    for direction in (-1, 1):
        maps = [lsc.halo_map(H, r, N, S, halo, direction, D) for r, N in shards]
        assert all(L.vrt_halo_bytes(W, H, bpp, C.byref(cs[i]), halo) == len(maps[i]) * rb for i in range(n))
        packed = _Packed(dev, [len(m) for m in maps], rb)
        check(L.vrt_pack_halo_batch(ctx, n, full_ptrs, packed.ptrs(), W, H, bpp, cs, halo, direction))
        engine.synchronize()
        packed.check([D.pack_np(fulls[i], maps[i]) for i in range(n)], maps, f"vrt_pack_halo_batch dir {direction}")
        packed.host = packed.t.cpu().numpy()
        dst_ptrs, dst, poison = unpack_into_poison(L.vrt_unpack_halo_batch, packed, maps, halo, direction)
    if null_at is not None:
        # a NULL image pointer behind the first launch's images: refused, and nothing is copied -- not the first 64 images either
        # (the targets are the full-size planes of the last unpack, poisoned again: large enough for either direction)
        dst.copy_(torch.from_numpy(poison))
        src = packed.ptrs()
        src[null_at] = None
        assert L.vrt_unpack_halo_batch(ctx, n, src, dst_ptrs, W, H, bpp, cs, halo, 1) == 1 and b"NULL image pointer" in L.vrt_last_error()
        assert L.vrt_unpack_rows_batch(ctx, n, src, dst_ptrs, W, H, bpp, cs) == 1
        dst_ptrs[null_at] = None
        assert L.vrt_pack_halo_batch(ctx, n, full_ptrs, dst_ptrs, W, H, bpp, cs, halo, 1) == 1
        assert L.vrt_pack_rows_batch(ctx, n, full_ptrs, dst_ptrs, W, H, bpp, C.byref(one)) == 1
        engine.synchronize()
        assert (dst.cpu().numpy() == poison).all(), "a refused call copied rows"


@pytest.mark.parametrize("bpp", [4, 16])
@pytest.mark.parametrize("n", lsc.COPY_SIZES)
def test_row_copies_past_64_images(vrt, engine, n, bpp):
    """64, 65 and 130 images per call; image 64 + k never has the shard of image k."""
    _copies(vrt, engine, n, bpp, lsc.copy_shards(n), np.random.default_rng(100 * n + bpp), null_at=70 if n > 70 else None)


def test_row_copies_with_packed_buffers_of_different_heights(vrt, engine):
    """Shards of 1, 2, 3 and 4 ranks in one call: every packed buffer has the size vrt_halo_bytes / vrt_shard_rows states for its
    own shard, and nothing is written behind it.  (A launch used to take its height from the largest buffer of its 64 images and
    zero-filled the padding rows of every image up to that height: past the end of the shorter buffers.)"""
    _copies(vrt, engine, 70, 4, lsc.mixed_shards(70), np.random.default_rng(5))


# ---- C. segment lengths of the verified kernels ---------------------------------------------------------------------------------

def _dev_planes(engine, planes):
    return [torch.from_numpy(np.array(a)).to(engine.torch_device) for a in planes]          # (a copy: the shared planes are read-only)


def _den_settings(vrt, W, H, iterations, step, mode):
    st = vrt.VoxelRenderSettings(targetResolution=(W, H))
    d = st.denoiserSettings
    d.iterations, d.stepWidth, d.mode = iterations, step, mode
    return st


@pytest.mark.parametrize("R", [2, 3, 4, 5])
def test_pair_kernel_at_every_segment_length(vrt, oracle, engine, R):
    """k_denoise_pair with the segment count set through "denoise_pair_wgs": the minimum 2 R, 3 R, a long segment, a single segment over
    the frame, and about 48 rows with a last segment of one row.  The exact mode (canonical taps: the as-shipped ones never take this
    kernel) equals the oracle whatever the length; which pixels are evaluated twice is the pixel's affair, so the counts agree
    between the lengths; VRT_DENOISE_FAST gives one image whatever the length."""
    cases = [c for c in lsc.PAIR_CASES if c.R == R]
    assert engine.option("denoise_pair") == 1 and engine.option("denoise_verified") == 1 and engine.option("denoise_p0") == 1
    for W, H in sorted({(c.W, c.H) for c in cases}):
        truth = dsc.gbuffer("hostile", W, H)
        c_, n_, p_ = _dev_planes(engine, truth)
        exp = oracle.denoise(*truth, iterations=2, step_width0=float(R - 1), mode=0)
        counts, fast = {}, {}
        for c in (c for c in cases if (c.W, c.H) == (W, H)):
            for mode in (0, vrt.DENOISE_FAST):
                st = _den_settings(vrt, W, H, c.iterations, c.step, mode)
                with engine.options(denoise_pair_wgs=c.pair_wgs, denoise_count=1):
                    stage = vrt.DenoiserStage(engine, st)
                    assert stage.guard(1) <= 0.02
                    got = stage.record(c_, n_, p_).cpu().numpy().copy()
                    if mode == 0:
                        counts[c.seg_rows] = [stage.redone(i) for i in range(c.iterations)]
                        bad = np.flatnonzero((got != exp).any((1, 2)))
                        assert bad.size == 0, f"R {R}, {W}x{H}, seg_rows {c.seg_rows} (last {c.last}): rows {bad[:12].tolist()} differ from the oracle"
                    else:
                        fast[c.seg_rows] = got
        assert len(counts) >= 2 and len({tuple(v) for v in counts.values()}) == 1, (R, W, H, counts)
        assert next(iter(counts.values()))[1] > 0
        first = next(iter(fast.values()))
        for seg, img in fast.items():
            bad = np.flatnonzero((img != first).any((1, 2)))
            assert bad.size == 0, f"R {R}, {W}x{H}, VRT_DENOISE_FAST: seg_rows {seg} differs from seg_rows {next(iter(fast))} in rows {bad[:12].tolist()}"
        assert np.abs(first.astype(np.int32) - exp.astype(np.int32)).max() <= 1        # (one weighted pass: the stated bound)


@pytest.mark.parametrize("case", lsc.VER_CASES, ids=[c.id for c in lsc.VER_CASES])
def test_ver_kernel_in_segments_longer_than_eight_rows(vrt, oracle, engine, case):
    """k_denoise_ver ("denoise_pair" = 0, "denoise_p0" = 0) on wide, low frames: segments of 12, 16 and 20 rows, last segments of one
    row, tap offsets 1, 2, 3, 5, the as-shipped taps, pass 0 -- each against the oracle."""
    truth = dsc.gbuffer("hostile", case.W, case.H)
    st = _den_settings(vrt, case.W, case.H, case.iterations, case.step, case.mode)
    with engine.options(denoise_pair=0, denoise_p0=0):
        stage = vrt.DenoiserStage(engine, st)
        assert all(stage.guard(i) <= 0.02 for i in range(1, case.iterations))
        got = stage.record(*_dev_planes(engine, truth)).cpu().numpy()
    exp = oracle.denoise(*truth, iterations=case.iterations, step_width0=case.step, mode=case.mode)
    bad = np.flatnonzero((got != exp).any((1, 2)))
    assert bad.size == 0, f"{case.id} {case.passes}: rows {bad[:12].tolist()} differ from the oracle"


def test_sharded_pair_kernel_with_a_forced_segment_count(vrt, oracle, engine):
    """Strips of 64 rows take k_denoise_pair; "denoise_pair_wgs" = 21 makes it walk them in segments of 21 rows, the last of one row.
    Poisoned planes: own rows equal the oracle, rows beyond the halo are untouched (dsc.run_rank)."""
    c = lsc.ShardPairCase
    truth = dsc.gbuffer("hostile", c.W, c.H)
    exp = oracle.denoise(*truth, iterations=c.iterations, step_width0=c.step, mode=0)
    st = _den_settings(vrt, c.W, c.H, c.iterations, c.step, 0)
    halo = dsc.halo_rows(c.iterations, c.step)
    rng = np.random.default_rng(19)
    with engine.options(denoise_pair_wgs=c.pair_wgs):
        for rank in range(c.nranks):
            own = dsc.owned_rows(c.H, rank, c.nranks, c.strip_rows)
            for kind in dsc.POISONS:
                got = dsc.run_rank(vrt, engine, st, dsc.poisoned(truth, c.H, rank, c.nranks, c.strip_rows, halo, kind, rng), rank, c.nranks,
                                   c.strip_rows, halo, rng)
                bad = (got[own] != exp[own]).any((1, 2))
                assert not bad.any(), f"rank {rank}, poison {kind}: own rows {own[bad]} differ from the oracle"


# ---- D. the tolerance kernels that nothing else launches ------------------------------------------------------------------------

_gb = {}


def _rendered_gbuffer(vrt, engine, res):
    """The G-buffer of tests/test_gpu_denoise.py's fast tests (a rendered frame), once per size."""
    if res not in _gb:
        vol = vrt.synthetic.floating_cubes(48, seed=4, count=60)
        sc = vrt.VoxelScene.from_dense(engine, vol, metallic_palette(vrt), sky=vrt.synthetic.sky_gradient(64, 32), noise=vrt.synthetic.blue_noise_standin(64))
        st = vrt.VoxelRenderSettings(targetResolution=res)
        st.fsrSetttings.enable = False
        st.occlusionSettings.numSamples = 2
        gb = vrt.GeometryStage(engine, st, sc).record(camera_push(vrt, (48, 48, 48), res))
        engine.synchronize()
        g = gb.numpy()
        _gb[res] = tuple(np.ascontiguousarray(g[k]) for k in ("color8", "normal8", "position"))
    return _gb[res]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("step", lsc.FAST_STEPS)
@pytest.mark.parametrize("size", lsc.FAST_SIZES)
def test_fast_kernel_within_one_code_per_pass(vrt, oracle, engine, size, step, mode):
    """k_denoise_fast ("denoise_verified" = 0 with VRT_DENOISE_FAST), tiles of 8 and of 16 rows ("denoise_th16"): the bound of
    include/vrt.h, at most one RGBA8 code per channel and weighted pass, measured as test_fast_denoise_within_one_code_per_pass
    measures it (the earlier passes are the oracle's: at most iterations - 1 codes end to end); pass 0 is exact.  Both tile heights
    run ONE body per pixel -- the tile height only says which rows a wave takes -- so their images are also bit-identical.  They
    are not k_denoise_ver's FAST image: that kernel sums the position distance in another order and takes the colour and normal
    distances as integers, so only the bound relates the two."""
    truth = _rendered_gbuffer(vrt, engine, size)
    planes = _dev_planes(engine, truth)
    worst = 0
    with engine.options(denoise_verified=0):
        st = _den_settings(vrt, size[0], size[1], 1, step, mode | vrt.DENOISE_FAST)
        got = vrt.DenoiserStage(engine, st).record(*planes).cpu().numpy()
        assert (got == oracle.denoise(*truth, iterations=1, step_width0=step, mode=mode)).all(), "pass 0 is exact"
        for iterations in lsc.FAST_ITERATIONS:
            exp = oracle.denoise(*truth, iterations=iterations, step_width0=step, mode=mode)
            st = _den_settings(vrt, size[0], size[1], iterations, step, mode | vrt.DENOISE_FAST)
            out = {}
            for th16 in (0, 1):
                with engine.options(denoise_th16=th16):
                    out[th16] = vrt.DenoiserStage(engine, st).record(*planes).cpu().numpy().copy()
                d = int(np.abs(out[th16].astype(np.int32) - exp.astype(np.int32)).max())
                worst = max(worst, d)
                print(f"k_denoise_fast {size} step {step} mode {mode} iterations {iterations} th16 {th16}: {d} codes")
                assert d <= iterations - 1, (iterations, th16, d)
            assert (out[0] == out[1]).all(), (iterations, int((out[0] != out[1]).sum()))
    print("k_denoise_fast: worst difference", worst, "codes")


def test_sharded_fast_lds_kernel_within_one_code(vrt, oracle, engine):
    """The same mode with a shard: the FAST form of k_denoise_lds (extended strips of 16 rows).  Poisoned planes; one weighted pass
    on an exact pass 0: own rows at most one code from the oracle, rows beyond the halo untouched."""
    W, H, N, S, it, step = lsc.FAST_SHARD
    halo = dsc.halo_rows(it, step)
    rng = np.random.default_rng(23)
    with engine.options(denoise_verified=0):
        for gkind in ("hostile", "smooth"):
            truth = dsc.gbuffer(gkind, W, H)
            for mode in (0, 1):
                exp = oracle.denoise(*truth, iterations=it, step_width0=step, mode=mode)
                st = _den_settings(vrt, W, H, it, step, mode | vrt.DENOISE_FAST)
                for rank in range(N):
                    own = dsc.owned_rows(H, rank, N, S)
                    for kind in dsc.POISONS:
                        got = dsc.run_rank(vrt, engine, st, dsc.poisoned(truth, H, rank, N, S, halo, kind, rng), rank, N, S, halo, rng)
                        d = int(np.abs(got[own].astype(np.int32) - exp[own].astype(np.int32)).max())
                        assert d <= it - 1, (gkind, mode, rank, kind, d)


@pytest.mark.parametrize("mode", [0, 1])
def test_fast_ver_kernel_within_one_code_per_pass(vrt, oracle, engine, mode):
    """VRT_DENOISE_FAST with "denoise_pair" = 0: the weighted passes take the cheap half of k_denoise_ver alone (FLAG = false), with the
    tap offsets 2, 3 and 5 at compile time and 4 at run time (lsc.FAST_VER_SETTINGS).  The bound of include/vrt.h, non-finite
    positions included: at most one code per channel and weighted pass, so iterations - 1 codes end to end against the oracle."""
    W, H = lsc.FAST_VER_SIZE
    for gkind in ("hostile", "smooth"):
        truth = dsc.gbuffer(gkind, W, H)
        planes = _dev_planes(engine, truth)
        for iterations, step in lsc.FAST_VER_SETTINGS:
            exp = oracle.denoise(*truth, iterations=iterations, step_width0=step, mode=mode)
            st = _den_settings(vrt, W, H, iterations, step, mode | vrt.DENOISE_FAST)
            with engine.options(denoise_pair=0):
                got = vrt.DenoiserStage(engine, st).record(*planes).cpu().numpy()
            d = int(np.abs(got.astype(np.int32) - exp.astype(np.int32)).max())
            print(f"k_denoise_ver FAST {gkind} mode {mode} iterations {iterations} step {step}: {d} codes")
            assert d <= iterations - 1, (gkind, mode, iterations, step, d)


# ---- E. tags_async ----------------------------------------------------------------------------------------------------------------

def test_tags_async_changes_no_plane(vrt, oracle, engine):
    """Ten launches without a synchronise, behind a busy stream, on a scene whose tile tags differ from pose to pose -- facing the
    volume, facing away, grazing it, a sharded launch, a batch of 11 through the table (the tag kernel waits for the upload), a larger
    batch (the tag buffer is allocated anew), single frames again -- with "tags_async" = 2 (the tags of every launch on the second
    stream), 1 (while the stream is busy) and 0.  Every plane equals the tags_async = 0 run, the single frames the oracle.  Each value
    runs on a context of its own, so each allocates its tag buffers within the sequence."""
    dims, res = lsc.TAGS_DIMS, lsc.TAGS_RES
    vol = vrt.synthetic.floating_cubes(dims[0], **lsc.TAGS_CUBES)
    pal = metallic_palette(vrt)
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    scene = vrt.VoxelScene.from_dense(engine, vol, pal, sky=sky, noise=noise)
    st = _settings(vrt, res, "default")
    st.occlusionSettings.numSamples = lsc.TAGS_AO
    stc = st.to_c()
    seq = [(kind, pushes, vrt._capi.Shard(*sh) if sh is not None else None) for kind, pushes, sh in lsc.tags_sequence(vrt, camera_push)]
    assert len(seq) >= 8 and len(seq[5][1]) > len(seq[4][1]) > lsc.MAX_BATCH
    engine.synchronize()

    def run(value):
        eng = vrt.Engine(0)
        try:
            eng.set_option("tags_async", value)
            assert eng.option("tags_async") == value and eng.option("tile_tags") == 1
            outs = [Planes(vrt, eng.torch_device, len(pushes), res) for _, pushes, _ in seq]
            arrs = [(vrt._capi.Push * len(pushes))(*pushes) for _, pushes, _ in seq]
            eng.synchronize()
            keep = _stall(eng.torch_device)
            for (kind, pushes, sh), out, arr in zip(seq, outs, arrs):
                if kind == "single":
                    vrt._capi.check(vrt.lib().vrt_render_geometry(eng.ctx, scene.handle, C.byref(arr[0]), C.byref(stc), C.byref(out.c[0]),
                                                                  C.byref(sh) if sh is not None else None))
                else:
                    vrt._capi.check(vrt.lib().vrt_render_geometry_batch(eng.ctx, scene.handle, len(pushes), arr, C.byref(stc), out.c, None))
            eng.synchronize()
            del keep
            return [o.bytes() for o in outs]
        finally:
            eng.set_option("tags_async", 0)
            eng.destroy()

    ref = run(0)
    tags = [r["mask8"] != 0 for r in ref]
    assert not tags[1].any() and tags[0].mean() > 0.05 and tags[2].any() and not tags[2].all()       # away, facing, grazing
    assert (ref[3]["mask8"][0, :16] == lsc.POISON).all() and (ref[3]["mask8"][0, 16:32] != lsc.POISON).all()
    osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    for k, (kind, pushes, sh) in enumerate(seq):
        if kind == "single" and sh is None:
            bad = compare_planes(Planes.typed(ref[k], 0), oracle.render(osn, pushes[0], oracle.params_from(stc), planes=NAMES, nthreads=8), NAMES)
            assert not bad, (k, bad)
    for value in (2, 1):
        got = run(value)
        for k in range(len(seq)):
            _same(got[k], ref[k], NAMES, f"tags_async = {value}, launch {k} ({seq[k][0]})")
