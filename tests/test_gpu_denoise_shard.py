"""The sharded denoiser (vrt_denoise with a vrt_shard), every kernel path, against the oracle on poisoned frames.

Every rank of a case gets planes that hold the truth on its own rows +- vrt_denoise_halo_rows(), clipped to the frame, and poison
everywhere else (tests/denoise_shard_common.py; tests/test_denoise_shard_cpu.py proves on the oracle alone that this is enough and
no more than enough).  Its own rows of the result must equal oracle.denoise of the TRUE full frame bit for bit under both poisons,
and in both ping-pong targets every row farther than the halo from all of its strips must still hold the bytes it was pre-filled
with: a sharded pass reads own rows +- halo and writes own rows +- (halo - 1) at most.

What launch_denoise_pass selects (csrc/vrt_denoise_plan.h), with R the tap offset i * stepWidth + 1 of pass i, ext the sum of the
reaches of the later passes and per = strip_rows + 2 ext the height of an extended strip -- the `path` of a case names what it is for:

  pass 0, canonical taps, verified, "denoise_p0" = 1                                   k_denoise_p0            p0-ver, pair, edges, ...
  R integral in 2 .. 5, canonical taps, verified, "denoise_pair" = 1, per >= 64        k_denoise_pair<.., R>   pair
  R integral in 1 .. 5, verified (guard <= the limit; pass 0 always)                   k_denoise_ver           p0-ver, pair-p0-off,
      (as-shipped taps: <SHIPPED>, pass 0: <.., PASS0>; VRT_DENOISE_FAST: FLAG = false)                        shipped, halo-gt-strip, edges,
                                                                                                               pair (per < 64), bilinear (4)
  R integral in 1 .. 5, not verified ("denoise_verified" = 0 or the guard too large),
      per a multiple of 4                                                              k_denoise_lds           literal, guard
  anything else (R not integral, R > 5, per not a multiple of 4)                       k_denoise               literal, bilinear, halo-gt-strip
  k_denoise_fast is never taken with a shard.
tests/test_launch_shapes_cpu.py asks the library's own routing (csrc/vrt_denoise_plan.h) which of these every pass of every case takes.
"""
import numpy as np
import pytest
import torch

import denoise_shard_common as dsc

pytestmark = pytest.mark.gpu

_exp = {}


def _expected(oracle, case, gkind, **over):
    kw = dict(case.oracle_kw(), **over)
    key = (gkind, case.W, case.H) + tuple(sorted(kw.items()))
    if key not in _exp:
        _exp[key] = oracle.denoise(*dsc.gbuffer(gkind, case.W, case.H), **kw)
    return _exp[key]


def _settings(vrt, case, iterations=None, mode=None):
    st = vrt.VoxelRenderSettings(targetResolution=(case.W, case.H))
    d = st.denoiserSettings
    d.iterations, d.stepWidth = case.iterations if iterations is None else iterations, case.step
    d.mode = case.mode if mode is None else mode
    d.phiColor0, d.phiNormal0, d.phiPos0 = case.phis
    return st


@pytest.mark.parametrize("case", dsc.CASES, ids=[c.id for c in dsc.CASES])
def test_sharded_denoise_owned_rows_are_the_oracles(vrt, oracle, engine, case):
    W, H, N, S, halo = case.W, case.H, case.nranks, case.strip_rows, case.halo
    truth = dsc.gbuffer("hostile", W, H)
    exp = _expected(oracle, case, "hostile")
    st = _settings(vrt, case)
    if case.guard_too_large:                                   # 0.02: kDenGuardMax, the largest guard a pass is verified with
        assert vrt.DenoiserStage(engine, st).guard(1) > 0.02
    rng = np.random.default_rng(11)
    with engine.options(**case.options):
        for rank in range(N):
            own = dsc.owned_rows(H, rank, N, S)
            for kind in dsc.POISONS:
                got = dsc.run_rank(vrt, engine, st, dsc.poisoned(truth, H, rank, N, S, halo, kind, rng), rank, N, S, halo, rng)
                bad = (got[own] != exp[own]).any((1, 2))
                assert not bad.any(), f"rank {rank}, poison {kind}: own rows {own[bad]} differ from the oracle"


@pytest.mark.parametrize("gkind", ["hostile", "smooth"])
@pytest.mark.parametrize("nranks,strip_rows", [(2, 16), (3, 16), (2, 64)])
@pytest.mark.parametrize("size", [(63, 49), (117, 130)])
def test_sharded_fast_denoise_within_one_code(vrt, oracle, engine, gkind, nranks, strip_rows, size):
    """VRT_DENOISE_FAST with a shard: k_denoise_ver / k_denoise_pair with FLAG = false and, under "denoise_verified" = 0,
    k_denoise_lds<.., true>.  One weighted pass on an exact pass 0: at most ONE RGBA8 code per channel from the oracle's exact image
    (the bound of include/vrt.h, as test_fast_denoise_single_weighted_pass_bound holds the unsharded kernels to); pass 0 alone is
    exact.  No bound over several weighted passes is asserted: the header states none beyond "per pass".

    Measured on an MI355X: hostile G-buffer 0 codes, smooth G-buffer 0 codes at 63x49 and 1 code at 117x130, for every shard.  (The
    hostile frames first missed the bound by up to 208 codes, every offending pixel with a NaN, infinite or -3e19 position among
    its taps: the one merged exponential made a NaN position distance a NaN weight where the shader's fminf(exp(NaN), 1) is 1.  The
    fast kernels now give that term 0, sharded or not.)"""
    W, H = size
    truth = dsc.gbuffer(gkind, W, H)
    rng = np.random.default_rng(13)
    worst = 0
    for mode in (0, 1):
        case = dsc.Case("fast", W, H, nranks, strip_rows, 2, 2.0, mode=mode)
        exact = {it: _expected(oracle, case, gkind, iterations=it) for it in (1, 2)}
        for verified in (1, 0):
            with engine.options(denoise_verified=verified):
                for it in (1, 2):
                    st = _settings(vrt, case, iterations=it, mode=mode | vrt.DENOISE_FAST)
                    halo = dsc.halo_rows(it, 2.0)
                    for rank in range(nranks):
                        own = dsc.owned_rows(H, rank, nranks, strip_rows)
                        for kind in dsc.POISONS:
                            got = dsc.run_rank(vrt, engine, st, dsc.poisoned(truth, H, rank, nranks, strip_rows, halo, kind, rng), rank, nranks, strip_rows, halo, rng)
                            d = np.abs(got[own].astype(np.int32) - exact[it][own].astype(np.int32))
                            dmax = int(d.max()) if d.size else 0
                            worst = max(worst, dmax)
                            if dmax > it - 1:                     # how many of the offending pixels have a non-finite position among their taps
                                bad = np.zeros((H, W), bool); bad[own] = d.max(-1) > it - 1
                                nf = ~np.isfinite(truth[2]).all(-1)
                                pad = np.pad(nf, 3, mode="edge")
                                near = np.zeros((H, W), bool)
                                for dy in (0, 3, 6):
                                    for dx in (0, 3, 6):
                                        near |= pad[dy:dy + H, dx:dx + W]
                                note = f"{int(bad.sum())} pixels over the bound, {int((bad & near).sum())} of them with a non-finite position among their taps"
                            assert dmax <= it - 1, f"mode {mode} verified {verified} iterations {it} rank {rank} poison {kind}: {dmax} codes; {note}"
    print(f"sharded fast denoise {gkind} {W}x{H} ({nranks}, {strip_rows}): worst difference {worst} codes")


def test_sharded_fuzz_sweep(vrt, oracle, engine):
    """30 random cases of tests/fuzz_denoise.py's sharded sweep (sizes, phis, steps, modes, G-buffer kinds, shards, poisons)."""
    import fuzz_denoise
    ranks = fuzz_denoise.run_sharded(vrt, oracle, engine, 30, seed=2027)
    assert ranks >= 60


def test_halo_batch_copies_against_the_row_maps(vrt, engine):
    """vrt_pack_halo_batch / vrt_unpack_halo_batch called directly: three images with three different shards in one launch, against
    distributed.halo_row_map + pack_np; unpacked into poisoned planes, only the mapped rows change.  And vrt_pack_rows for a rank
    without a strip: all padding, nothing read."""
    import ctypes as C
    D, L, ctx, dev = vrt.distributed, vrt.lib(), engine.ctx, engine.torch_device
    W, H, N, S = 50, 40, 3, 16
    P = C.c_void_p
    rng = np.random.default_rng(17)
    shards = (vrt._capi.Shard * N)(*[vrt._capi.Shard(r, N, S) for r in range(N)])
    for bpp in (4, 16):
        fulls = [rng.integers(0, 256, (H, W * bpp), dtype=np.uint8) for _ in range(N)]
        dfull = [torch.from_numpy(f).to(dev) for f in fulls]
        for direction in (-1, 1):
            for halo in (1, 7, 16):
                rows = D.max_local_strips(H, N, S) * halo
                assert all(L.vrt_halo_bytes(W, H, bpp, C.byref(shards[r]), halo) == rows * W * bpp for r in range(N))
                packed = [torch.full((rows, W * bpp), 77, dtype=torch.uint8, device=dev) for _ in range(N)]
                vrt._capi.check(L.vrt_pack_halo_batch(ctx, N, (P * N)(*[t.data_ptr() for t in dfull]), (P * N)(*[t.data_ptr() for t in packed]),
                                                      W, H, bpp, shards, halo, direction))
                engine.synchronize()
                maps = [D.halo_row_map(H, r, N, S, halo, direction) for r in range(N)]
                for r in range(N):
                    got, want = packed[r].cpu().numpy(), D.pack_np(fulls[r], maps[r])
                    ok = maps[r] >= 0
                    assert ok.any() and (got[ok] == want[ok]).all(), (bpp, direction, halo, r)
                    assert np.isin(got[~ok], (0, 77)).all()                       # padding rows: zeros or untouched, never image bytes
                poison = [rng.integers(0, 256, (H, W * bpp), dtype=np.uint8) for _ in range(N)]
                dst = [torch.from_numpy(q).to(dev) for q in poison]
                vrt._capi.check(L.vrt_unpack_halo_batch(ctx, N, (P * N)(*[t.data_ptr() for t in packed]), (P * N)(*[t.data_ptr() for t in dst]),
                                                        W, H, bpp, shards, halo, direction))
                engine.synchronize()
                for r in range(N):
                    want = poison[r].copy()
                    D.unpack_np(D.pack_np(fulls[r], maps[r]), want, maps[r])
                    assert (dst[r].cpu().numpy() == want).all(), (bpp, direction, halo, r)
    # a rank without a strip (rank 3 of (4, 16) on 40 rows): its packed buffer is padding throughout, and no row of the source is needed
    sh = vrt._capi.Shard(3, 4, S)
    assert len(D.owned_rows(H, 3, 4, S)) == 0 and (D.packed_row_map(H, 3, 4, S) < 0).all()
    src = torch.from_numpy(rng.integers(1, 256, (H, W * 4), dtype=np.uint8)).to(dev)
    packed = torch.full((D.packed_rows(H, 4, S), W * 4), 77, dtype=torch.uint8, device=dev)
    vrt._capi.check(L.vrt_pack_rows(ctx, src.data_ptr(), packed.data_ptr(), W, H, 4, C.byref(sh)))
    back = torch.full((H, W * 4), 55, dtype=torch.uint8, device=dev)
    vrt._capi.check(L.vrt_unpack_rows(ctx, packed.data_ptr(), back.data_ptr(), W, H, 4, C.byref(sh)))
    engine.synchronize()
    assert np.isin(packed.cpu().numpy(), (0, 77)).all()
    assert (back == 55).all()
