"""Shared by tests/test_segments_cpu.py and tests/test_gpu_segments.py: the volumes, the rays and the distance limits of the segment
queries' tests, and the expected records -- tests/segment_reference.py once it has been held to the oracle."""
import numpy as np

import segment_reference as SR
from ray_query_common import query_rays

N_RAYS = 5000
BUDGETS = (512, 37, 1)
# (seed, dims, fill) of test_ray_query_cpu.VOLUMES: multiples of 8, so the same content goes into bricks
VOLUMES = [(11, (40, 32, 56), 0.002), (12, (64, 64, 64), 0.02), (14, (16, 8, 8), 0.1)]
T_CLASSES = ("exact", "below", "half", "double", "inf", "zero", "minus_one", "nan")


def make_volume(seed, dims, fill):
    from test_ray_query_cpu import make_volume as mv
    return mv(seed, dims, fill)


def draw_t_max(rng, t_hit, hit):
    """One limit per ray and the class it was drawn from (index into T_CLASSES): t_hit exactly, the float below it, half and twice
    of it, +inf, 0, -1 and NaN; a miss has no t_hit, and where one of the first four classes falls on it the limit is a random
    positive number."""
    n = len(t_hit)
    cls = rng.integers(0, len(T_CLASSES), n)
    t = np.asarray(t_hit, np.float32)
    tm = np.select([cls == 0, cls == 1, cls == 2, cls == 3, cls == 4, cls == 5, cls == 6],
                   [t, np.nextafter(t, np.float32(-np.inf)), np.float32(0.5) * t, np.float32(2.0) * t, np.float32(np.inf), np.float32(0.0), np.float32(-1.0)],
                   np.float32(np.nan)).astype(np.float32)
    rnd = rng.uniform(0.01, 100.0, n).astype(np.float32)
    return np.where(~hit & (cls < 4), rnd, tm).astype(np.float32), cls


def pick_segment_seed(oracle, osn, dims, first):
    """A seed whose batch holds, at max_steps 512 and decided on the oracle's hits and the drawn classes alone: at least 5 % of rays
    each that hit and keep the hit whatever its distance (exact, double, inf), that hit and lose it (below, minus_one, nan), and that miss
    anyway; and at least 100 hits each in the classes exact and below.  Returns (seed, starts, dirs, class of every ray, the oracle's
    records at 512)."""
    share = None
    for seed in range(first, first + 40):
        starts, dirs = query_rays(np.random.default_rng(seed), N_RAYS, dims)
        orc = SR.oracle_trace(oracle, osn, starts, dirs, 512)
        hit = orc["material"] != 0
        cls = np.random.default_rng(seed + 7).integers(0, len(T_CLASSES), N_RAYS)
        share = (float((hit & np.isin(cls, (0, 3, 4))).mean()), float((hit & np.isin(cls, (1, 6, 7))).mean()), float((~hit).mean()),
                 int((hit & (cls == 0)).sum()), int((hit & (cls == 1)).sum()))
        if min(share[:3]) >= 0.05 and min(share[3:]) >= 100:
            return seed, starts, dirs, cls, orc
    raise AssertionError(f"no seed in {first} .. {first + 39} meets the conditions on {dims}: {share}")


def segment_case(oracle, seed, dims, fill, budgets=BUDGETS):
    """One volume's test data: the volume, 5000 rays, their limits, and for every budget the reference's trace -- held to the oracle
    here, ray by ray -- and the expected records under the limits."""
    vol = make_volume(seed, dims, fill)
    osn = oracle.OracleScene(vol, np.zeros((256, 5), np.float32))
    ray_seed, starts, dirs, cls, orc512 = pick_segment_seed(oracle, osn, dims, 100 * seed)
    ref, exp = {}, {}
    assert 512 in budgets
    for ms in budgets:
        ref[ms] = SR.trace(vol, starts, dirs, ms)
        orc = orc512 if ms == 512 else SR.oracle_trace(oracle, osn, starts, dirs, ms)
        bad = SR.differs_from_oracle(ref[ms], orc)
        assert bad.size == 0, ("segment_reference differs from the oracle", dims, ms, bad[:5], starts[bad[:3]], dirs[bad[:3]])
    hit = ref[512]["material"] != 0
    t_max, cls2 = draw_t_max(np.random.default_rng(ray_seed + 7), ref[512]["t"], hit)
    assert (cls2 == cls).all()
    for ms in budgets:
        exp[ms] = SR.segment_records(ref[ms], t_max)
    return {"vol": vol, "dims": dims, "ray_seed": ray_seed, "starts": starts, "dirs": dirs, "t_max": t_max, "cls": cls, "ref": ref, "exp": exp}


def planes_differ(got, exp, names=("material", "pos", "voxel", "normal", "t")):
    """Indices of the rays whose records differ, pos and t by bit pattern."""
    bad = np.zeros(len(exp[names[0]]), bool)
    for k in names:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (k, g.shape, e.shape, g.dtype, e.dtype)
        if k in ("pos", "t"):
            g, e = g.view(np.uint32), e.view(np.uint32)
        d = g != e
        bad |= d if d.ndim == 1 else d.any(axis=1)
    return np.flatnonzero(bad)
