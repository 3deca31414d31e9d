"""What the sharded-denoiser tests share (tests/test_denoise_shard_cpu.py on the oracle alone, tests/test_gpu_denoise_shard.py on the
kernels, tests/fuzz_denoise.py's sharded sweep): the strip arithmetic restated in a few lines of numpy, the poisoned frames, the
G-buffer makers and the table of cases.

The idea.  A rank's planes hold the truth on the rows it owns and on `vrt_denoise_halo_rows()` rows either side of every owned strip
(what the ring exchange delivers), clipped to the frame.  In a real run every other row is zeros left by an unrendered G-buffer:
position 0 and normal 0 read as sky, whose weight against almost every neighbour is 0, so a pass that read a row too far would not
change a byte.  Here every other row is POISON chosen to enter a sum at full weight:

  "colour"  colour = 255 - truth in all four channels, normal and position true.  The geometric weights of a stray tap are those of
            the true frame (1 in pass 0, whose weights are all 1), so the wrong colour enters wherever the right one would have.
  "nan"     every position component NaN, normal and colour random bytes.  fminf(exp(NaN), 1) = 1 by the numeric spec, so the
            position weight of a stray tap is 1 and the garbage colour is taken whole.

The oracle filters the TRUE full frame; a sharded pass that reads, or fails to produce, a row it should not differs from it on an
owned row.
"""
import numpy as np

import fuzz_denoise

POISONS = ("colour", "nan")


# ---- strip arithmetic, restated (cross-checked against vrt.distributed and vrt_denoise_halo_rows by the CPU test) ----------------

def reaches(iterations, step_width):
    """Rows a tap of pass i reaches: ceil(i * stepWidth + 1), in float32 as the stage computes the tap offset."""
    return [int(np.ceil(np.float32(i) * np.float32(step_width) + np.float32(1.0))) for i in range(iterations)]


def halo_rows(iterations, step_width):
    return sum(reaches(iterations, step_width))


def strips(H, rank, nranks, strip_rows):
    """[(first row, one past the last)] of the strips `rank` owns: strip g = rows g*strip_rows .., owner g % nranks."""
    return [(b, min(H, b + strip_rows)) for b in range(rank * strip_rows, H, nranks * strip_rows)]


def owned_rows(H, rank, nranks, strip_rows):
    s = strips(H, rank, nranks, strip_rows)
    return np.concatenate([np.arange(b, e) for b, e in s]) if s else np.zeros(0, np.int64)


def band_mask(H, rank, nranks, strip_rows, band):
    """bool[H]: the rows within `band` rows of an owned strip, clipped to the frame.  band: rows, or (rows above, rows below)."""
    up, down = (band, band) if np.isscalar(band) else band
    m = np.zeros(H, bool)
    for b, e in strips(H, rank, nranks, strip_rows):
        m[max(0, b - up):min(H, e + down)] = True
    return m


def poisoned(planes, H, rank, nranks, strip_rows, band, kind, rng):
    """The (colour, normal, position) planes as `rank` holds them: the truth within `band` rows of an owned strip, poison elsewhere."""
    color, nrm, pos = (a.copy() for a in planes)
    bad = ~band_mask(H, rank, nranks, strip_rows, band)
    n = int(bad.sum())
    if kind == "colour":
        color[bad] = 255 - color[bad]
    elif kind == "nan":
        W = color.shape[1]
        color[bad] = rng.integers(0, 256, (n, W, 4), dtype=np.uint8)
        nrm[bad] = rng.integers(-128, 128, (n, W, 4)).astype(np.int8)
        pos[bad] = np.float32(np.nan)
    else:
        raise ValueError(kind)
    return color, nrm, pos


# ---- one rank on the GPU ---------------------------------------------------------------------------------------------------------

def run_rank(vrt, engine, st, planes, rank, nranks, strip_rows, halo, rng):
    """One sharded record() on pre-filled targets.  Returns the result image (host), or raises if a row beyond the halo was written."""
    import torch
    dev = engine.torch_device
    H, W = planes[0].shape[:2]
    c, n, p = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in planes)
    fill = [rng.integers(0, 256, (H, W, 4), dtype=np.uint8) for _ in range(2)]
    stage = vrt.DenoiserStage(engine, st)
    stage._targets = [torch.from_numpy(f).to(dev) for f in fill]
    out = stage.record(c, n, p, vrt._capi.Shard(rank, nranks, strip_rows))
    engine.synchronize()
    got = out.cpu().numpy()
    keep = ~band_mask(H, rank, nranks, strip_rows, halo)
    for k in range(2):
        t = stage._targets[k].cpu().numpy()
        assert (t[keep] == fill[k][keep]).all(), f"rank {rank}: target {k} written beyond the halo, rows {np.flatnonzero((t != fill[k]).any((1, 2)) & keep)}"
        if not len(strips(H, rank, nranks, strip_rows)):
            assert (t == fill[k]).all(), f"rank {rank} owns no strip, target {k} written"
    return got


# ---- G-buffers -------------------------------------------------------------------------------------------------------------------

def _hostile_gbuffer(rng, W, H):
    """Random codes in every channel (alpha and w included, SNORM -128 too), positions clustered so that the weights are
    neither 0 nor 1, a sprinkling of equal neighbours, huge, infinite and NaN positions."""
    color = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    flat = rng.random((H, W, 1)) < 0.3
    color = np.where(flat, color // 64 * 64, color).astype(np.uint8)             # flat patches: sums whose mean is a code exactly
    nrm = rng.choice(np.array([-128, -127, -90, -73, -1, 0, 1, 73, 90, 127], np.int8), (H, W, 4))
    nrm = np.where(rng.random((H, W, 1)) < 0.5, np.array([0, 127, 0, 0], np.int8), nrm).astype(np.int8)
    pos = rng.uniform(0, 64, (H, W, 4)).astype(np.float32)
    pos = (np.round(pos * 4) / 4 + rng.normal(0, 0.05, (H, W, 4))).astype(np.float32)
    pos[..., 3] = np.where(rng.random((H, W)) < 0.9, 0.0, pos[..., 3])
    odd = rng.random((H, W))
    pos[odd < 0.002] = np.float32(np.nan)
    pos[(odd >= 0.002) & (odd < 0.004)] = np.float32(np.inf)
    pos[(odd >= 0.004) & (odd < 0.006)] = np.float32(-3e19)
    pos[(odd >= 0.006) & (odd < 0.3)] = 0.0                                       # sky
    return color, nrm, pos


_cache = {}


def gbuffer(gkind, W, H):
    """The true planes of a W x H frame, made once per session and never written to: "hostile" (_hostile_gbuffer) or "smooth"
    (fuzz_denoise.make_gbuffer kind 0, rendered-like).  The seed is the size, so both test files see the same frame."""
    key = (gkind, W, H)
    if key not in _cache:
        rng = np.random.default_rng(W * 4099 + H)
        planes = _hostile_gbuffer(rng, W, H) if gkind == "hostile" else fuzz_denoise.make_gbuffer(rng, W, H, 0)
        planes = tuple(np.ascontiguousarray(a) for a in planes)
        for a in planes:
            a.setflags(write=False)
        _cache[key] = planes
    return _cache[key]


# ---- the cases -------------------------------------------------------------------------------------------------------------------

DEFAULT_PHIS = (20.4, 1e-2, 1e-1)


class Case:
    """One row instance of the table in tests/test_gpu_denoise_shard.py."""

    def __init__(self, path, W, H, nranks, strip_rows, iterations, step, mode=0, phis=DEFAULT_PHIS, options=None, guard_too_large=False):
        self.path, self.W, self.H, self.nranks, self.strip_rows = path, W, H, nranks, strip_rows
        self.iterations, self.step, self.mode, self.phis = iterations, step, mode, phis
        self.options = dict(options or {})
        self.guard_too_large = guard_too_large

    @property
    def halo(self):
        return halo_rows(self.iterations, self.step)

    @property
    def id(self):
        opts = "".join(f"-{k[8:]}{v}" for k, v in sorted(self.options.items()))
        return f"{self.path}-{self.W}x{self.H}-n{self.nranks}s{self.strip_rows}-i{self.iterations}w{self.step:g}-m{self.mode}{opts}"

    def oracle_kw(self):
        return dict(iterations=self.iterations, step_width0=self.step, mode=self.mode,
                    phi_color0=self.phis[0], phi_normal0=self.phis[1], phi_pos0=self.phis[2])


def _cross(path, settings, shards, sizes, **kw):
    return [Case(path, W, H, n, s, it, st, **kw) for (it, st) in settings for (n, s) in shards for (W, H) in sizes]


def cases():
    c = []
    # k_denoise_p0 sharded + k_denoise_ver (extended strip < 64 rows)
    c += _cross("p0-ver", [(2, 2.0), (3, 2.0), (3, 1.0), (3, 0.0)], [(2, 16), (3, 16), (4, 32)], [(62, 33), (63, 49), (125, 130), (37, 17)])
    # k_denoise_pair sharded, tap offsets 2 .. 5; (2, 48) with three passes: extended strips of 64 (p0), 58 and 48 rows (ver)
    c += _cross("pair", [(2, 1.0), (2, 2.0), (3, 2.0), (2, 3.0), (2, 4.0)], [(2, 64), (3, 64), (2, 48), (2, 80)],
                [(58, 129), (59, 129), (117, 200), (54, 65)])
    # the same frames with the pair and pass-0 kernels switched off
    for opts in ({"denoise_pair": 0}, {"denoise_p0": 0}, {"denoise_pair": 0, "denoise_p0": 0}):
        for (n, s) in ((3, 16), (2, 64)):
            for (W, H) in ((63, 49), (117, 200)):
                c.append(Case("pair-p0-off", W, H, n, s, 3, 2.0, options=opts))
    # the as-shipped taps (k_denoise_ver<SHIPPED>, pass 0: <SHIPPED, PASS0>)
    c += _cross("shipped", [(2, 2.0), (3, 1.0)], [(2, 16), (3, 32), (2, 64)], [(65, 50), (130, 97)], mode=1)
    # the exact kernels: tiled k_denoise_lds where the extended strip is a multiple of 4 rows, untiled k_denoise where it is not
    for mode in (0, 1):
        c += _cross("literal", [(2, 2.0), (3, 2.0), (2, 1.0)], [(2, 16), (3, 16)], [(70, 35), (64, 130)], mode=mode, options={"denoise_verified": 0})
    c.append(Case("literal", 70, 35, 2, 16, 3, 2.0, options={"denoise_verified": 0, "denoise_packed": 0}))
    c.append(Case("literal", 70, 35, 2, 16, 3, 2.0, mode=1, options={"denoise_verified": 0, "denoise_packed": 0}))
    # (48 rows = 3 whole strips over 2 ranks, an extended strip of 22 rows: the untiled launch's last block has rows to spare)
    c.append(Case("literal", 70, 48, 2, 16, 2, 2.0, options={"denoise_verified": 0}))
    # non-integral steps: the bilinear k_denoise (pass 0 is k_denoise_p0 all the same, and pass 2 of (3, 1.5) has the integral tap offset 4:
    # k_denoise_ver)
    c += _cross("bilinear", [(2, 2.5), (2, 0.75), (3, 1.5)], [(2, 16), (3, 16)], [(70, 50)])
    c.append(Case("bilinear", 70, 48, 2, 16, 2, 1.5))
    # a guard too large to verify with: weighted passes fall to k_denoise_lds
    c.append(Case("guard", 70, 50, 2, 16, 2, 2.0, phis=(1e-4, 1e-4, 1e-4), guard_too_large=True))
    # frame edges: a rank without a strip, frames shorter than the halo and than a strip, a last strip of one row, whole strips
    for (it, st) in ((2, 2.0), (3, 2.0)):
        for W in (1, 64, 100):
            for (n, s, H) in ((4, 16, 40), (2, 16, 5), (3, 32, 5), (2, 16, 33), (3, 32, 33), (2, 16, 65), (3, 32, 65), (5, 16, 80)):
                c.append(Case("edges", W, H, n, s, it, st))
    # a halo larger than a strip: the extended regions of a rank's own strips overlap
    c += _cross("halo-gt-strip", [(5, 2.0), (6, 1.0)], [(2, 16), (3, 16)], [(100, 130)])
    return c


CASES = cases()
