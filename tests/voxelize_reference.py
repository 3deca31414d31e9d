"""The definition of vrt_scene_voxelize in Python integers (numpy arrays of dtype object, whose elements are Python ints: no
product can overflow).  Nothing here is shared with csrc/vrt_voxelize.h.

Positions are in sixteenths of a voxel.  Voxel (x, y, z) is the closed cube [16x, 16x+16]^3 with centre c = (16x+8, 16y+8, 16z+8)
and half-side 8.

SURFACE: voxel and triangle meet iff none of 13 axes separates them (closed comparisons): the three box axes, the triangle's
normal, and the nine cross products of an edge with a unit axis.
SOLID: a triangle with n_x == 0 flips nothing; otherwise, s = sign(n_x), it flips the voxel of centre c iff c is in the triangle's
yz-projection under the top-left rule and s * n.(c - v0) < 0.  A voxel is inside iff an odd number of triangles flip it."""
import numpy as np

UNIT, HALF = 16, 8
SURFACE, SOLID = 1, 2
SET, PAINT, ADD, REPLACE = 0, 1, 2, 3
MODES = {"set": SET, "paint": PAINT, "add": ADD, "replace": REPLACE}
FILLS = {"surface": SURFACE, "solid": SOLID, "both": SURFACE | SOLID}
COORD_MIN, COORD_MAX = -65536, 131072
MAX_SIDE = 512


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def ints(tri):
    return [tuple(int(t) for t in p) for p in tri]


def voxel_span(m, M):
    """the voxels whose closed cube [16x, 16x+16] meets [m, M]: lo..hi inclusive"""
    return -((-m) // UNIT) - 1, M // UNIT


def centres(lo, hi):
    """centres of voxels lo..hi (inclusive) as an object array"""
    return np.array([UNIT * x + HALF for x in range(lo, hi + 1)], dtype=object)


def _b(a):
    return np.asarray(a).astype(bool)


def meets_grid(tri, lo, hi):
    """SURFACE for every voxel of lo..hi (inclusive, per axis) -> bool [z][y][x]"""
    v = ints(tri)
    cx = centres(lo[0], hi[0]).reshape(1, 1, -1)
    cy = centres(lo[1], hi[1]).reshape(1, -1, 1)
    cz = centres(lo[2], hi[2]).reshape(-1, 1, 1)
    d = [(p[0] - cx, p[1] - cy, p[2] - cz) for p in v]
    shape = (cz.size, cy.size, cx.size)
    ok = np.ones(shape, bool)

    def interval(k):
        p = [k[0] * dj[0] + k[1] * dj[1] + k[2] * dj[2] for dj in d]
        r = HALF * (abs(k[0]) + abs(k[1]) + abs(k[2]))
        return _b(np.minimum(np.minimum(p[0], p[1]), p[2]) <= r) & _b(np.maximum(np.maximum(p[0], p[1]), p[2]) >= -r)
    for k in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        ok = ok & np.broadcast_to(interval(k), shape)
    n = cross(sub(v[1], v[0]), sub(v[2], v[0]))
    nd = n[0] * d[0][0] + n[1] * d[0][1] + n[2] * d[0][2]
    ok = ok & np.broadcast_to(_b(abs(nd) <= HALF * (abs(n[0]) + abs(n[1]) + abs(n[2]))), shape)
    for e in (sub(v[1], v[0]), sub(v[2], v[1]), sub(v[0], v[2])):
        for u in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
            ok = ok & np.broadcast_to(interval(cross(e, u)), shape)
    return ok


def meets(tri, x, y, z):
    """SURFACE for one voxel, in plain ints: the same 13 axes, written out per voxel"""
    v = ints(tri)
    c = (UNIT * x + HALF, UNIT * y + HALF, UNIT * z + HALF)
    d = [sub(p, c) for p in v]
    edges = (sub(v[1], v[0]), sub(v[2], v[1]), sub(v[0], v[2]))
    units = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
    axes = list(units) + [cross(e, u) for e in edges for u in units]
    for k in axes:
        p = [k[0] * dj[0] + k[1] * dj[1] + k[2] * dj[2] for dj in d]
        r = HALF * (abs(k[0]) + abs(k[1]) + abs(k[2]))
        if min(p) > r or max(p) < -r:
            return False
    n = cross(sub(v[1], v[0]), sub(v[2], v[0]))
    return abs(n[0] * d[0][0] + n[1] * d[0][1] + n[2] * d[0][2]) <= HALF * (abs(n[0]) + abs(n[1]) + abs(n[2]))


def flips_grid(tri, lo, hi):
    """SOLID: which voxels of lo..hi (inclusive) the triangle flips -> bool [z][y][x]"""
    v = ints(tri)
    shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    n = cross(sub(v[1], v[0]), sub(v[2], v[0]))
    if n[0] == 0:
        return np.zeros(shape, bool)
    s = 1 if n[0] > 0 else -1
    cy = centres(lo[1], hi[1]).reshape(1, -1)
    cz = centres(lo[2], hi[2]).reshape(-1, 1)
    inside = np.ones(shape[:2], bool)
    for a, b in ((v[0], v[1]), (v[1], v[2]), (v[2], v[0])):
        dy, dz = s * (b[1] - a[1]), s * (b[2] - a[2])
        E = dy * (cz - a[2]) - dz * (cy - a[1])
        tie = dz > 0 or (dz == 0 and dy < 0)
        inside = inside & (_b(E > 0) | (_b(E == 0) & tie))
    out = np.zeros(shape, bool)
    zs, ys = np.nonzero(inside)
    if zs.size:
        cx = centres(lo[0], hi[0]).reshape(1, -1)
        cyl = np.array([UNIT * (lo[1] + int(y)) + HALF for y in ys], dtype=object).reshape(-1, 1)
        czl = np.array([UNIT * (lo[2] + int(z)) + HALF for z in zs], dtype=object).reshape(-1, 1)
        plane = s * (n[0] * (cx - v[0][0]) + n[1] * (cyl - v[0][1]) + n[2] * (czl - v[0][2]))
        out[zs, ys, :] = _b(plane < 0)
    return out


def flips(tri, x, y, z):
    return bool(flips_grid(tri, (x, y, z), (x, y, z))[0, 0, 0])


def covered(vertices, triangles, fill, lo, size):
    """the covered set inside the bounds [lo, lo + size) (not clipped to any volume) -> bool [z][y][x]"""
    lo = [int(t) for t in lo]
    size = [int(t) for t in size]
    hi = [lo[a] + size[a] - 1 for a in range(3)]
    cover = np.zeros((size[2], size[1], size[0]), bool)
    parity = np.zeros((size[2], size[1], size[0]), bool)
    for t in triangles:
        tri = ints([vertices[int(i)] for i in t])
        span = [voxel_span(min(p[a] for p in tri), max(p[a] for p in tri)) for a in range(3)]
        if fill & SURFACE:
            l = [max(lo[a], span[a][0]) for a in range(3)]
            h = [min(hi[a], span[a][1]) for a in range(3)]
            if all(h[a] >= l[a] for a in range(3)):
                sl = tuple(slice(l[a] - lo[a], h[a] - lo[a] + 1) for a in (2, 1, 0))
                if (h[0] - l[0] + 1) * (h[1] - l[1] + 1) * (h[2] - l[2] + 1) <= 8:      # a few voxels: one by one is quicker than arrays
                    for z in range(l[2], h[2] + 1):
                        for y in range(l[1], h[1] + 1):
                            for x in range(l[0], h[0] + 1):
                                if not cover[z - lo[2], y - lo[1], x - lo[0]] and meets(tri, x, y, z):
                                    cover[z - lo[2], y - lo[1], x - lo[0]] = True
                else:
                    cover[sl] |= meets_grid(tri, l, h)
        if fill & SOLID:
            l = [lo[0]] + [max(lo[a], span[a][0]) for a in (1, 2)]
            h = [hi[0]] + [min(hi[a], span[a][1]) for a in (1, 2)]
            if all(h[a] >= l[a] for a in range(3)):
                sl = tuple(slice(l[a] - lo[a], h[a] - lo[a] + 1) for a in (2, 1, 0))
                parity[sl] ^= flips_grid(tri, l, h)
    return cover | parity


def clip_bounds(dims, bounds):
    """bounds (lo, size) cut to the volume -> (lo, size) or None"""
    lo, size = bounds
    l = [max(0, int(lo[a])) for a in range(3)]
    h = [min(int(dims[a]), int(lo[a]) + int(size[a])) for a in range(3)]
    if any(h[a] <= l[a] for a in range(3)):
        return None
    return l, [h[a] - l[a] for a in range(3)]


def mesh_bounds(vertices):
    """the mesh's own voxel bounds (every vertex counts) -> (lo, size)"""
    v = np.asarray(vertices).reshape(-1, 3)
    span = [voxel_span(int(v[:, a].min()), int(v[:, a].max())) for a in range(3)]
    return tuple(s[0] for s in span), tuple(s[1] - s[0] + 1 for s in span)


ZERO = {"covered": 0, "changed": 0, "lo": (0, 0, 0), "size": (0, 0, 0)}


def value(mode, old, vid, match):
    if mode == PAINT:
        return np.where(old != 0, vid, old)
    if mode == ADD:
        return np.where(old == 0, vid, old)
    if mode == REPLACE:
        return np.where(old == match, vid, old)
    return np.full_like(old, vid)


def voxelize(vol, vertices, triangles, vid, mode=SET, fill=SURFACE, bounds=None, match=0, cover=None):
    """-> (the volume after, the result as VoxelScene.voxelize returns it).  cover: a dict that keeps covered()'s arrays by
    (fill, lo, size) for callers that put the same mesh into several volumes"""
    D, H, W = vol.shape
    mode = MODES[mode] if isinstance(mode, str) else mode
    fill = FILLS[fill] if isinstance(fill, str) else fill
    cb = clip_bounds((W, H, D), mesh_bounds(vertices) if bounds is None else bounds)
    if cb is None:
        return vol.copy(), dict(ZERO)
    lo, size = cb
    key = (fill, tuple(lo), tuple(size))
    cov = cover[key] if cover is not None and key in cover else covered(vertices, triangles, fill, lo, size)
    if cover is not None:
        cover[key] = cov
    out = vol.copy()
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    old = vol[sl]
    new = np.where(cov, value(mode, old, vid, match), old).astype(np.uint8)
    out[sl] = new
    ch = new != old
    res = dict(ZERO)
    res["covered"] = int(cov.sum())
    if ch.any():
        zs, ys, xs = np.nonzero(ch)
        mn = (int(xs.min()), int(ys.min()), int(zs.min()))
        mx = (int(xs.max()), int(ys.max()), int(zs.max()))
        res.update(changed=int(ch.sum()), lo=tuple(lo[a] + mn[a] for a in range(3)), size=tuple(mx[a] - mn[a] + 1 for a in range(3)))
    return out, res
