"""Shared by tests/test_ray_query_cpu.py and tests/test_gpu_ray_query.py: the ray mix of tests/test_traverse_host.py without the one
case the ray-query contract leaves open, and the oracle's record of a batch in the layout of vrt_ray_hits."""
import numpy as np


def query_rays(rng, n, dims):
    """test_traverse_host._rays (starts outside and inside, unnormalised directions, zero components, lattice ties) minus the
    excluded case: a zero direction component whose origin component is exactly 0 or exactly the volume's size on that axis
    (boxIntersection multiplies 0 by infinity there, include/vrt.h) -- such an origin is moved half a voxel along that axis."""
    from test_traverse_host import _rays
    starts, dirs = _rays(rng, n, dims)
    size = np.array(dims, np.float32)
    open_case = (dirs == 0.0) & ((starts == 0.0) | (starts == size[None, :]))
    starts = np.where(open_case, starts + np.float32(0.5), starts).astype(np.float32)
    assert not ((dirs == 0.0) & ((starts == 0.0) | (starts == size[None, :]))).any()
    assert np.isfinite(starts).all() and np.isfinite(dirs).all()
    return np.ascontiguousarray(starts), np.ascontiguousarray(dirs)


def oracle_records(oracle, osn, starts, dirs, max_steps, with_steps=False):
    """vo_trace_ray of every ray as the four planes of vrt_ray_hits, plus the class of every ray: 0 = hit, 1 = left the volume,
    2 = exhausted max_steps (the loop ran max_steps iterations without a hit).  with_steps: also the voxel fetches of every ray
    (a hit in the loop's k-th iteration has fetched k voxels)."""
    n = len(starts)
    mat = np.zeros(n, np.uint8); pos = np.zeros((n, 3), np.float32); vox = np.zeros((n, 3), np.int32); nrm = np.zeros((n, 3), np.int8)
    cls = np.zeros(n, np.uint8); steps = np.zeros(n, np.uint32)
    for i in range(n):
        h = oracle.trace_ray(osn, starts[i], dirs[i], max_steps)
        steps[i] = h.steps
        if h.material != 0:
            mat[i] = h.material
            pos[i] = list(h.pos)
            vox[i] = list(h.voxel)
            step = np.sign(np.asarray(dirs[i], np.float32)).astype(np.int32)
            nrm[i] = [-step[a] if (h.mask >> a) & 1 else 0 for a in range(3)]
            # (the oracle's own normal is this vector normalised)
            assert (np.sign(np.array(list(h.normal), np.float32)).astype(np.int32) == nrm[i]).all()
        else:
            cls[i] = 2 if h.steps >= max_steps else 1
    if with_steps:
        return {"material": mat, "pos": pos, "voxel": vox, "normal": nrm}, cls, steps
    return {"material": mat, "pos": pos, "voxel": vox, "normal": nrm}, cls


def planes_differ(got, exp, names=("material", "pos", "voxel", "normal")):
    """Indices of the rays whose records differ, pos by bit pattern."""
    bad = np.zeros(len(exp["material"]), bool)
    for k in names:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape and g.dtype == e.dtype, (k, g.shape, e.shape, g.dtype, e.dtype)
        if k == "pos":
            g, e = g.view(np.uint32), e.view(np.uint32)
        d = g != e
        bad |= d if d.ndim == 1 else d.any(axis=1)
    return np.flatnonzero(bad)


def bricks_of(vol):
    """A dense volume [z, y, x] with dimensions that are multiples of 8 as (grid, pool) of vrt_scene_from_bricks."""
    D, H, W = vol.shape
    nbz, nby, nbx = D // 8, H // 8, W // 8
    grid = np.zeros((nbz, nby, nbx), np.uint32); pool = []
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                b = vol[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8]
                if b.any():
                    pool.append(b.copy()); grid[bz, by, bx] = len(pool)
    return grid, (np.stack(pool) if pool else np.zeros((0, 8, 8, 8), np.uint8))


# ---- the finite-ray contract at its edges ------------------------------------------------------------------------------------
# Ray classes the built-in pinhole can never produce (tests/test_ray_query_cpu.py on the host build, tests/test_gpu_ray_query_edges.py
# on the GPU).  Every class keeps clear of the set include/vrt.h leaves open, by the predicate open_set below.
EDGE_CLASSES = ("axis1", "axis2", "negzero", "zero", "ortho_grid", "scaled", "far", "tiny", "lattice_in")
# Where a class cannot be generated, or cannot hold one of the two outcomes, on a volume -- (class, dims): (what is missing, why)
EDGE_IMPOSSIBLE = {
    ("lattice_in", (1, 1, 1)): ("class", "no integer lies strictly between 0 and 1: the class has no ray on this volume"),
}


def recip_inf(d):
    """1 / d overflows in fp32: d is +-0 or |d| <= 2^-128 (roughly; decided by the division itself, denormals preserved)."""
    with np.errstate(divide="ignore", over="ignore"):
        return np.isinf(np.float32(1.0) / np.asarray(d, np.float32))


def open_set(starts, dirs, dims):
    """The rays the contract of vrt_trace_rays leaves open (include/vrt.h, items (1) .. (4)), as (components [n, 3], rays [n]).  A
    component d is flat when 1 / d overflows.
      components -- (1) flat, and the origin component exactly 0 or the volume's size (boxIntersection: 0 * inf);
                    (2) flat, negative and non-zero, and the origin component an integer (sideDist: 0 * inf);
      rays       -- (3) all three flat and boxIntersection's test passes with tmin = tmax = +inf, so that its point is origin + inf * d:
                    some axis has both its planes at t = +inf (d = +flat and the origin below 0, or d = -flat and the origin above
                    the size) and no axis has both at -inf (the other way round).  With such an axis tmax = -inf, the test fails and
                    the ray is a defined miss from its own origin; with neither the origin is inside;
                    (4) not (0, 0, 0), and the largest |d| below 2^-68: a sideDist may overflow within max_steps (< 2^32) -- the
                    sideDist that steps is the smallest, at most (max_steps + 1) / max|d|, and adding a deltaDist (< 2^128) to less
                    than 2^100 does not round up to infinity -- and where all three are subnormal GLSL may flush them."""
    starts, dirs = np.asarray(starts, np.float32), np.asarray(dirs, np.float32)
    size = np.array(dims, np.float32)[None, :]
    flat = recip_inf(dirs)
    neg = np.signbit(dirs)
    comp = (flat & ((starts == 0.0) | (starts == size))) | (flat & (dirs < 0.0) & (starts == np.floor(starts)))
    below, above = starts < 0.0, starts > size
    plus = (~neg & below) | (neg & above)                    # both planes of the axis at t = +inf
    minus = (~neg & above) | (neg & below)                   # ... at t = -inf
    o3 = flat.all(axis=1) & plus.any(axis=1) & ~minus.any(axis=1)
    largest = np.abs(dirs).max(axis=1)
    o4 = (largest > 0.0) & (largest < np.float32(2.0 ** -68))
    return comp, o3 | o4


def _zero_origins(rng, n, dims, vol, negative):
    """Origins for the direction (+0, +0, +0) (negative: (-0, -0, -0)): a third each inside solid cells, inside empty cells (as far
    as the volume has them) and outside the volume on the side where boxIntersection is defined (open_set, (3)): one component
    beyond the size (negative: below 0), the others anywhere around the volume."""
    size = np.array(dims, np.float64)
    o = _targets(rng, n, dims, vol, 0.5)
    out = _origins(rng, n, dims, 0.0)
    a = rng.integers(0, 3, n)
    far_side = size[a] * (1.0 + rng.uniform(0.01, 1.0, n))
    out[np.arange(n), a] = -(far_side - size[a]) if negative else far_side
    return np.where((rng.random(n) < 1.0 / 3)[:, None], out, o)


def _targets(rng, n, dims, vol, solid_frac):
    """Points of the volume to aim at: uniform, and (where the volume is known and holds any) a share inside solid voxels."""
    t = rng.uniform([0, 0, 0], dims, (n, 3))
    if vol is not None and vol.any():
        z, y, x = np.nonzero(vol)
        pick = rng.integers(0, len(x), n)
        at = np.stack([x[pick], y[pick], z[pick]], axis=1) + rng.uniform(0.05, 0.95, (n, 3))
        t = np.where((rng.random(n) < solid_frac)[:, None], at, t)
    return t


def _origins(rng, n, dims, inside_frac=0.3):
    size = np.array(dims, np.float64)
    o = rng.uniform(-size, 2 * size, (n, 3))
    return np.where((rng.random(n) < inside_frac)[:, None], rng.uniform(0 * size, size, (n, 3)), o)


def _half_of_them_on_half_integers(rng, o):
    return np.where((rng.random(len(o)) < 0.5)[:, None], np.floor(o) + 0.5, o)


def _axis1(rng, n, dims, vol):
    size = np.array(dims, np.float64)
    a = rng.integers(0, 3, n)
    o = _targets(rng, n, dims, vol, 0.3)                                     # the two other coordinates: a column of the volume ...
    beside = rng.random(n) < 0.1
    o = np.where(beside[:, None], _origins(rng, n, dims, 0.0), o)            # ... or, for a tenth, anywhere around it
    along = np.where(rng.random(n) < 0.3, rng.uniform(0, 1, n), np.where(rng.random(n) < 0.5, rng.uniform(-1, 0, n), rng.uniform(1, 2, n))) * size[a]
    o[np.arange(n), a] = along
    d = np.zeros((n, 3))
    d[np.arange(n), a] = rng.choice([-1.0, 1.0], n) * np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.3, 2.0, n))
    return _half_of_them_on_half_integers(rng, o), d


def _axis2(rng, n, dims, vol):
    t = _targets(rng, n, dims, vol, 0.3)
    o = _origins(rng, n, dims)
    a = rng.integers(0, 3, n)
    keep = rng.random(n) < 0.85                                              # the origin lies in the slab of its target's cell along the zero axis
    o[np.arange(n), a] = np.where(keep, t[np.arange(n), a], o[np.arange(n), a])
    d = t - o
    d /= np.linalg.norm(d, axis=1)[:, None] + 1e-9
    d *= np.where(rng.random(n) < 0.15, rng.uniform(0.3, 2.0, n), 1.0)[:, None]
    d[np.arange(n), a] = 0.0
    return _half_of_them_on_half_integers(rng, o), d


def ortho_grid_rays(dims, axis, sign, gw, gh):
    """The rays of an axis-aligned orthographic view: a gw x gh lattice of origins on a plane 3.5 voxels in front of the face the view
    looks at, reaching min(2, size / 2) past the volume on every side, all with the direction sign * e_axis exactly.  Row-major."""
    size = np.array(dims, np.float64)
    u, v = [b for b in range(3) if b != axis]
    mu, mv = min(2.0, size[u] / 2), min(2.0, size[v] / 2)
    cu = (np.arange(gw) + 0.5) * ((size[u] + 2 * mu) / gw) - mu
    cv = (np.arange(gh) + 0.5) * ((size[v] + 2 * mv) / gh) - mv
    o = np.zeros((gh, gw, 3))
    o[..., u] = cu[None, :]; o[..., v] = cv[:, None]
    o[..., axis] = -3.5 if sign > 0 else size[axis] + 3.5
    d = np.zeros((gh, gw, 3)); d[..., axis] = float(sign)
    return o.reshape(-1, 3), d.reshape(-1, 3)


def _ortho_grid(rng, n, dims):
    per = -(-n // 6)
    gw = max(1, int(np.sqrt(per * 2))); gh = -(-per // gw)
    parts = [ortho_grid_rays(dims, axis, sign, gw, gh) for axis in range(3) for sign in (1, -1)]
    o = np.concatenate([p[0][:per] for p in parts])[:n]; d = np.concatenate([p[1][:per] for p in parts])[:n]
    return o, d


def _far(rng, n, dims, vol):
    # e uniform in 4 .. 30 for half of the rays; 4 .. 7.5 for the other half: past 10^7.5 voxels a float origin's ulp is wider than the
    # volume's cells, so with e uniform over the whole range no more than an eighth of the rays could resolve a voxel at all and the
    # class could not hold 5 % hits on the sparse volumes
    size = np.array(dims, np.float64)
    e = np.where(rng.random(n) < 0.5, rng.uniform(4.0, 30.0, n), rng.uniform(4.0, 7.5, n))
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    o = (size / 2 + (10.0 ** e)[:, None] * u).astype(np.float32)             # the origin as the query will see it ...
    d = _targets(rng, n, dims, vol, 0.5) - o.astype(np.float64)             # ... aimed in double, rounded once
    d /= np.linalg.norm(d, axis=1)[:, None]
    return o, d


def _tiny(rng, n, dims, vol):
    size = np.array(dims, np.float64)
    t = _targets(rng, n, dims, vol, 0.3)
    o = _origins(rng, n, dims)
    d = t - o
    d /= np.linalg.norm(d, axis=1)[:, None] + 1e-9
    o, d = o.astype(np.float32), d.astype(np.float32)
    # one or two components become subnormal: 1 .. 23 significant bits, either sign; those below 2^21 have an infinite reciprocal
    sub = np.zeros((n, 3), bool)
    sub[np.arange(n), rng.integers(0, 3, n)] = True
    second = rng.random(n) < 0.4
    sub[np.arange(n)[second], rng.integers(0, 3, n)[second]] = True
    sub[sub.all(axis=1), 0] = False                                          # (cannot happen with two draws; kept as the class's definition)
    bits = (rng.integers(1, 1 << 23, (n, 3)) >> rng.integers(0, 23, (n, 3))).astype(np.uint32)
    bits = np.maximum(bits, 1) | (rng.integers(0, 2, (n, 3)).astype(np.uint32) << np.uint32(31))
    d = np.where(sub, bits.view(np.float32), d)
    # the ray does not move along such an axis: its origin lies in the volume's slab there (a tenth do not: they miss)
    slab = rng.uniform(0, 1, (n, 3)) * size
    o = np.where(sub & (rng.random((n, 3)) < 0.9), np.where(rng.random((n, 3)) < 0.5, t, slab), o)
    return o, d


def _lattice_in(rng, n, dims, vol):
    size = np.array(dims, np.int64)
    assert (size >= 2).all(), EDGE_IMPOSSIBLE[("lattice_in", (1, 1, 1))][1]
    o = rng.integers(1, size, (n, 3)).astype(np.float64)                     # 1 .. size - 1: strictly inside
    t = _targets(rng, n, dims, vol, 0.3)
    d = t - o
    d /= np.linalg.norm(d, axis=1)[:, None] + 1e-9
    kind = rng.integers(0, 4, n)
    sg = rng.choice([-1.0, 1.0], (n, 3))
    d = np.where((kind == 1)[:, None], sg * rng.choice([0.5, 1.0, 2.0], n)[:, None], d)                # three-axis ties
    two = sg * np.array([1.0, 1.0, 1.0]); two[np.arange(n), rng.integers(0, 3, n)] *= rng.choice([0.25, 0.5], n)
    d = np.where((kind == 2)[:, None], two, d)                                                          # two-axis ties
    z = d.copy(); z[np.arange(n), rng.integers(0, 3, n)] = 0.0
    d = np.where((kind == 3)[:, None], z, d)                                                            # one zero component
    return o, d


def edge_rays(rng, n, dims, cls, vol=None):
    """float32 starts and dirs [n, 3] of one class of EDGE_CLASSES on a volume of `dims` (vol, where given, only steers a share of
    the rays towards solid voxels so that sparse volumes see hits; what a ray meets is for the oracle to say):
      axis1       exactly two zero components; origins inside and outside, half of them on half-integer coordinates
      axis2       exactly one zero component
      negzero     axis1, axis2 (two fifths each) and zero with their zeros written as -0.0.  Which march can tell sign(-0.0) = -1
                  from 0: none through axis1 / axis2 (an axis with infinite deltaDist never holds the minimum beside a finite one, so
                  its rayStep is never used); through the zero part only a march that moves by rayStep on the three-way tie at +inf --
                  the GPU's look-up loop (its index increments are rayStep) and the oracle's literal loop.  VRT_TRAVERSAL_DF and the
                  brick march, all the host build has, move by the sideDist travelled and stand still either way
      zero        direction (0, 0, 0); origins inside solid cells, inside empty cells and outside (_zero_origins)
      ortho_grid  axis-aligned orthographic views along +-x, +-y, +-z, one lattice after the other (ortho_grid_rays)
      scaled      query_rays' directions times 2^k, k uniform in -60 .. 60 (exact)
      far         origins 10^e from the volume's centre, aimed at a point of the volume in double and rounded once (_far on e)
      tiny        one or two direction components subnormal, some with an infinite reciprocal, the others ordinary
      lattice_in  origins on integer coordinates strictly inside the volume; ordinary, tying and one-zero directions
    A component in the open set (open_set: (1), (2)) has its origin moved half a voxel along that axis, as query_rays does; no class
    may lose more than 10 % of its rays that way, and none generates a ray of (3) or (4)."""
    dims = tuple(int(v) for v in dims)
    if cls == "axis1":
        o, d = _axis1(rng, n, dims, vol)
    elif cls == "axis2":
        o, d = _axis2(rng, n, dims, vol)
    elif cls == "negzero":
        h = 2 * n // 5
        (o1, d1), (o2, d2) = _axis1(rng, h, dims, vol), _axis2(rng, h, dims, vol)
        o3 = _zero_origins(rng, n - 2 * h, dims, vol, True)                 # (the rest as in `zero`)
        o, d = np.concatenate([o1, o2, o3]), np.concatenate([d1, d2, np.zeros((n - 2 * h, 3))])
        d = np.where(d == 0.0, -0.0, d)
    elif cls == "zero":
        o, d = _zero_origins(rng, n, dims, vol, False), np.zeros((n, 3))
    elif cls == "ortho_grid":
        o, d = _ortho_grid(rng, n, dims)
    elif cls == "scaled":
        o, d = query_rays(rng, n, dims)
        d = np.ldexp(d, rng.integers(-60, 61, n)[:, None]).astype(np.float32)
    elif cls == "far":
        o, d = _far(rng, n, dims, vol)
    elif cls == "tiny":
        o, d = _tiny(rng, n, dims, vol)
    elif cls == "lattice_in":
        o, d = _lattice_in(rng, n, dims, vol)
    else:
        raise ValueError(cls)
    o, d = np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
    comp, rays = open_set(o, d, dims)
    assert not rays.any(), (cls, int(rays.sum()))
    assert comp.any(axis=1).mean() <= 0.10, (cls, comp.any(axis=1).mean())
    o = np.where(comp, o + np.float32(0.5), o).astype(np.float32)
    comp, rays = open_set(o, d, dims)
    assert not comp.any() and not rays.any()
    assert np.isfinite(o).all() and np.isfinite(d).all()
    if cls in ("axis1", "ortho_grid"):
        assert ((d == 0.0).sum(axis=1) == 2).all()
    if cls == "axis2":
        assert ((d == 0.0).sum(axis=1) == 1).all()
    if cls == "negzero":
        assert (d == 0.0).any(axis=1).all() and np.signbit(d[d == 0.0]).all()
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


# ---- the long volume: hits that need 850 .. 1100 iterations -------------------------------------------------------------------
LONG_DIMS = (1100, 8, 8)
LONG_BUDGETS = (1023, 1024, 1025, 2000)


def long_volume(mirrored=False):
    """1100 x 8 x 8: empty from x = 0 on, single voxels at x in 900 .. 1059 (each cell with probability 0.012, so that about one
    ray in seven along x gets through them), a solid slab from x = 1060 on.  mirrored: the same along -x."""
    rng = np.random.default_rng(1100)
    W, H, D = LONG_DIMS
    vol = np.zeros((D, H, W), np.uint8)
    vol[:, :, 900:1060] = (rng.random((D, H, 160)) < 0.012) * rng.integers(1, 256, (D, H, 160))
    vol[:, :, 1060:] = 9
    return np.ascontiguousarray(vol[:, :, ::-1]) if mirrored else vol


def long_rays(n, mirrored=False, dims=LONG_DIMS, axis=0, sign=None, along=((-3.0, 3.0),), margin=2.5, slopes=(0.002, 0.05), seed=1101):
    """n rays that start within three voxels of the x = 0 face, inside the volume or just outside it, and run along +x: seven in ten
    from the middle of the section with a slope of at most 0.002 against the axis (they stay inside the 8 x 8 section all the way), the others up to 3 degrees
    (they leave through a side).  mirrored: the same rays reflected to start at the far end and run along -x.
    Generalised (tests/extents_common.py): the volume `dims`, its long `axis`, `sign` of travel (-1 = mirrored), the ranges `along`
    the axis that ray i % len(along) starts in, measured from the face the rays leave behind, the `margin` the origins keep from
    the section's sides, and the two slope classes.  `sign`, where given (not None), decides the direction and `mirrored` is not
    looked at; the callers of the 1100 x 8 x 8 volume pass `mirrored` alone."""
    rng = np.random.default_rng(seed)
    if sign is not None:
        mirrored = sign < 0
    u, v = [b for b in range(3) if b != axis]
    lo, hi = (np.array([along[i % len(along)][k] for i in range(n)]) for k in (0, 1))
    o = np.empty((n, 3))
    o[:, axis], o[:, u], o[:, v] = rng.uniform(lo, hi, n), rng.uniform(margin, dims[u] - margin, n), rng.uniform(margin, dims[v] - margin, n)
    slope = np.where(rng.random(n) < 0.7, slopes[0], slopes[1])[:, None] * rng.uniform(-1, 1, (n, 2))
    d = np.empty((n, 3))
    d[:, axis], d[:, u], d[:, v] = 1.0, slope[:, 0], slope[:, 1]
    d *= rng.uniform(0.5, 2.0, n)[:, None]
    if mirrored:
        o[:, axis] = dims[axis] - o[:, axis]; d[:, axis] = -d[:, axis]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)
