"""The harness of tests/test_gpu_denoise_shard.py proved on the oracle alone, before any kernel is involved (no GPU).

For every case of the table (tests/denoise_shard_common.py) and every rank:

  Sufficiency.  oracle.denoise of the frame poisoned beyond `halo` rows of the rank's strips equals oracle.denoise of the true frame
      on the rank's own rows, bit for bit, under both poisons.  So vrt_denoise_halo_rows() is enough for the reference filter, and
      the values the GPU test expects of a rank that holds no more than that are the right ones.

  Bite.  With the truth kept one row short of the halo, at least one own pixel of the rank differs under the "colour" poison: the
      halo is tight and the poison is seen.  Asserted on the smooth G-buffer with the default phis and an integral step.  A row at
      exactly `halo` rows from a strip reaches an own row only through the one chain of outermost taps, one hop per pass, so the
      assertion needs a chain whose geometric weights do not vanish, and that is read off the input planes (_open_side): at some
      column every texel of the chain carries the same normal and all are sky (every weight 1) or, under the canonical taps with at
      most three passes, all are geometry (the position weight of a vertical hop of 2 i + 1 rows in pass i is
      exp(-i (0.05 (2 i + 1))^2 / 0.1): 1e-6 over the hops of five passes, nothing an RGBA8 code shows; the as-shipped taps hop
      diagonally, across a depth that changes with the column, and their position weight on geometry is 0).  Exempt are:
        - sides on which the frame's edge clips the band, so that no row lies at exactly `halo` rows from a strip of the rank (both
          sides of every strip: a rank whose band covers the frame, and frames shorter than the halo);
        - ranks none of whose sides has such a chain (the normals of the smooth G-buffer change every 8 rows, as the strips do);
        - iterations 0 (nothing is filtered) -- the table has none;
        - the lower side under the as-shipped taps, (-1, -1), (1, -1) and (0, 0), which only reach upwards: bite is asserted with the
          band shortened above only, and the opposite below -- rows under the strips are never read (a band of 0 rows is sufficient).
"""
import ctypes as C

import numpy as np
import pytest

import denoise_shard_common as dsc

_exp = {}


def _open_side(case, planes, rank, side):
    """Does a row at exactly `halo` rows above (side -1) / below (+1) a strip of `rank` lie in the frame outside the band of
    halo - 1 rows, with a chain of outermost taps to an own row whose geometric weights are not 0?  (module docstring)"""
    _, nrm, pos = planes
    H, W = nrm.shape[:2]
    r = dsc.reaches(case.iterations, case.step)
    short = dsc.band_mask(H, rank, case.nranks, case.strip_rows, case.halo - 1)
    shipped = (case.mode & 1) == 1
    x = np.arange(W)
    for b, e in dsc.strips(H, rank, case.nranks, case.strip_rows):
        y = b if side < 0 else e - 1
        far = y + side * case.halo
        if far < 0 or far >= H or short[far]:
            continue
        ys, xs = [y], [x]
        for i in range(case.iterations - 1, 0, -1):            # the hops of the weighted passes, last pass first
            ys.append(ys[-1] + side * r[i])
            xs.append(np.clip(xs[-1] + r[i], 0, W - 1) if shipped else x)
        n = np.stack([nrm[yy, xx].view(np.uint32)[:, 0] for yy, xx in zip(ys, xs)])
        sky = np.stack([(pos[yy, xx] == 0).all(-1) for yy, xx in zip(ys, xs)])
        same = (n == n[0]).all(0)
        if (same & sky.all(0)).any() or (not shipped and case.iterations <= 3 and (same & ~sky.any(0)).any()):
            return True
    return False


def _expected(oracle, case, gkind):
    key = (gkind, case.W, case.H, case.iterations, case.step, case.mode, case.phis)
    if key not in _exp:
        _exp[key] = oracle.denoise(*dsc.gbuffer(gkind, case.W, case.H), **case.oracle_kw())
    return _exp[key]


def test_strip_arithmetic_is_the_librarys(vrt):
    D = vrt.distributed
    for H in (1, 5, 16, 17, 33, 40, 80, 130, 200):
        for nranks, strip_rows in ((2, 16), (3, 16), (4, 32), (5, 16), (2, 64), (2, 80)):
            rows = [dsc.owned_rows(H, r, nranks, strip_rows) for r in range(nranks)]
            assert (np.sort(np.concatenate(rows)) == np.arange(H)).all()
            for r in range(nranks):
                assert (rows[r] == D.owned_rows(H, r, nranks, strip_rows)).all()
                m = dsc.band_mask(H, r, nranks, strip_rows, 0)
                assert (np.flatnonzero(m) == rows[r]).all()
    for iterations, step in sorted({(c.iterations, c.step) for c in dsc.CASES} | {(0, 2.0), (10, 5.0), (4, 0.3)}):
        ds = vrt._capi.DenoiserSettings(); vrt.lib().vrt_denoiser_settings_default(C.byref(ds))
        ds.iterations, ds.step_width = iterations, step
        assert vrt.lib().vrt_denoise_halo_rows(C.byref(ds)) == dsc.halo_rows(iterations, step), (iterations, step)


def test_the_table_reaches_what_it_names():
    """The shapes of the table against the launcher's selection rule (restated in tests/test_gpu_denoise_shard.py)."""
    def per(c, i):
        return c.strip_rows + 2 * sum(dsc.reaches(c.iterations, c.step)[i + 1:])
    by = {}
    for c in dsc.CASES:
        by.setdefault(c.path, []).append(c)
    assert all(per(c, i) < 64 for c in by["p0-ver"] for i in range(1, c.iterations))
    offs = {int(i * c.step + 1) for c in by["pair"] for i in range(1, c.iterations) if per(c, i) >= 64}
    assert offs == {2, 3, 4, 5}
    assert any(per(c, 1) == 58 and per(c, 2) == 48 for c in by["pair"])
    assert {per(c, i) % 4 == 0 for c in by["literal"] for i in range(c.iterations)} == {True, False}
    assert all(c.halo > c.strip_rows for c in by["halo-gt-strip"])
    assert any(len(dsc.strips(c.H, r, c.nranks, c.strip_rows)) == 0 for c in by["edges"] for r in range(c.nranks))
    assert any(c.H < c.halo and c.H < c.strip_rows for c in by["edges"])
    assert len({c.id for c in dsc.CASES}) == len(dsc.CASES)


@pytest.mark.parametrize("case", dsc.CASES, ids=[c.id for c in dsc.CASES])
def test_halo_is_sufficient_and_tight(oracle, case):
    W, H, N, S, halo = case.W, case.H, case.nranks, case.strip_rows, case.halo
    truth = dsc.gbuffer("hostile", W, H)
    exp = _expected(oracle, case, "hostile")
    shipped = (case.mode & 1) == 1
    rng = np.random.default_rng(7)
    for rank in range(N):
        own = dsc.owned_rows(H, rank, N, S)
        for kind in dsc.POISONS:
            got = oracle.denoise(*dsc.poisoned(truth, H, rank, N, S, halo, kind, rng), **case.oracle_kw())
            assert (got[own] == exp[own]).all(), (rank, kind)
    if case.step != int(case.step) or case.phis != dsc.DEFAULT_PHIS or case.iterations == 0:
        return
    smooth = dsc.gbuffer("smooth", W, H)
    sexp = _expected(oracle, case, "smooth")
    for rank in range(N):
        own = dsc.owned_rows(H, rank, N, S)
        sides = [sd for sd in ((-1,) if shipped else (-1, 1)) if _open_side(case, smooth, rank, sd)]
        if sides:
            band = (halo - 1, halo) if shipped else (halo - 1, halo - 1)
            got = oracle.denoise(*dsc.poisoned(smooth, H, rank, N, S, band, "colour", rng), **case.oracle_kw())
            assert (got[own] != sexp[own]).any(), rank
        if shipped and len(own):
            got = oracle.denoise(*dsc.poisoned(smooth, H, rank, N, S, (halo, 0), "colour", rng), **case.oracle_kw())
            assert (got[own] == sexp[own]).all(), rank


def test_bite_is_asserted_widely():
    """The exemptions must not hollow the assertion out: of the cases with an integral step, most have a rank that asserts it."""
    elig = [c for c in dsc.CASES if c.step == int(c.step) and c.phis == dsc.DEFAULT_PHIS]
    n = sum(1 for c in elig if any(_open_side(c, dsc.gbuffer("smooth", c.W, c.H), r, sd) for r in range(c.nranks) for sd in (-1, 1)
                                   if not ((c.mode & 1) and sd > 0)))
    assert 2 * n >= len(elig), (n, len(elig))
