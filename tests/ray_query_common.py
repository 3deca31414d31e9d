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


def oracle_records(oracle, osn, starts, dirs, max_steps):
    """vo_trace_ray of every ray as the four planes of vrt_ray_hits, plus the class of every ray: 0 = hit, 1 = left the volume,
    2 = exhausted max_steps (the loop ran max_steps iterations without a hit)."""
    n = len(starts)
    mat = np.zeros(n, np.uint8); pos = np.zeros((n, 3), np.float32); vox = np.zeros((n, 3), np.int32); nrm = np.zeros((n, 3), np.int8)
    cls = np.zeros(n, np.uint8)
    for i in range(n):
        h = oracle.trace_ray(osn, starts[i], dirs[i], max_steps)
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
