"""A restatement of csrc/vrt_brush.h for the tests: shapes, modes, clipping, the changed count, the tight box, stamps.

The shape predicates are evaluated in PYTHON INTEGERS (numpy arrays of dtype object, or plain loops): they cannot overflow, so
where the header's int64 arithmetic and this file disagree the header is wrong.  The predicates here are the bare inequalities
of the issue, evaluated wherever they are asked -- there is no bounding-box shortcut in `inside`, so a header whose bounds cut a
covered voxel away is caught.  Volumes are uint8 arrays indexed [z, y, x]; positions of shapes are in half voxels, the centre
of voxel (x, y, z) being (2x+1, 2y+1, 2z+1)."""
import numpy as np

BOX, ELLIPSOID, CAPSULE = 0, 1, 2
SET, PAINT, ADD, REPLACE = 0, 1, 2, 3
SHAPES = {"box": BOX, "ellipsoid": ELLIPSOID, "capsule": CAPSULE}
MODES = {"set": SET, "paint": PAINT, "add": ADD, "replace": REPLACE}
SKIP_EMPTY = 1
MAX_RADIUS, CAPSULE_MIN, CAPSULE_MAX, BOX_MAX_SIZE, STAMP_MAX_SIDE = 1024, -4096, 12288, 1 << 30, 512
PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))     # the source axis that feeds destination x, y, z
ORIENTS = [perm | flips << 3 for flips in range(8) for perm in range(6)]


def params(p):
    p = [int(v) for v in p]
    return p + [0] * (9 - len(p))


def shape_ok(shape, p):
    p = params(p)
    if shape == BOX:
        return all(1 <= s <= BOX_MAX_SIZE for s in p[3:6])
    if shape == ELLIPSOID:
        return all(1 <= r <= MAX_RADIUS for r in p[3:6])
    if shape == CAPSULE:
        return all(CAPSULE_MIN <= v <= CAPSULE_MAX for v in p[0:6]) and 1 <= p[6] <= MAX_RADIUS
    return False


def mode_ok(mode, vid, match):
    if mode == SET:
        return True
    if mode in (PAINT, ADD):
        return vid != 0
    if mode == REPLACE:
        return vid != match
    return False


def inside(shape, p, x, y, z):
    """The predicate in Python integers.  x, y, z: integers, or object arrays of integers (the result is then a bool array)."""
    p = params(p)
    if shape == BOX:
        r = True
        for v, lo, n in zip((x, y, z), p[0:3], p[3:6]):
            r = r & (v >= lo) & (v < lo + n)
        return _bool(r)
    P = [2 * x + 1, 2 * y + 1, 2 * z + 1]
    if shape == ELLIPSOID:
        d = [P[a] - p[a] for a in range(3)]
        rx2, ry2, rz2 = p[3] * p[3], p[4] * p[4], p[5] * p[5]
        return _bool(d[0] * d[0] * (ry2 * rz2) + d[1] * d[1] * (rx2 * rz2) + d[2] * d[2] * (rx2 * ry2) <= rx2 * ry2 * rz2)
    a, b, r = p[0:3], p[3:6], p[6]
    e = [b[i] - a[i] for i in range(3)]
    L2 = sum(v * v for v in e)
    da = [P[i] - a[i] for i in range(3)]
    db = [P[i] - b[i] for i in range(3)]
    q = da[0] * e[0] + da[1] * e[1] + da[2] * e[2]
    da2 = da[0] * da[0] + da[1] * da[1] + da[2] * da[2]
    db2 = db[0] * db[0] + db[1] * db[1] + db[2] * db[2]
    first = _bool(q <= 0) | (L2 == 0)
    second = _bool(q >= L2)
    return np.where(first, _bool(da2 <= r * r), np.where(second, _bool(db2 <= r * r), _bool(da2 * L2 - q * q <= r * r * L2))) if isinstance(first, np.ndarray) \
        else bool(da2 <= r * r if first else (db2 <= r * r if second else da2 * L2 - q * q <= r * r * L2))


def _bool(v):
    return v.astype(bool) if isinstance(v, np.ndarray) else bool(v)


def bounds(shape, p):
    """The voxel box [lo, hi) that holds every covered voxel: per axis the voxels whose centre lies within the shape's extent."""
    p = params(p)
    lo, hi = [], []
    for a in range(3):
        if shape == BOX:
            lo.append(p[a]); hi.append(p[a] + p[3 + a])
            continue
        m, M = (p[a] - p[3 + a], p[a] + p[3 + a]) if shape == ELLIPSOID else (min(p[a], p[3 + a]) - p[6], max(p[a], p[3 + a]) + p[6])
        lo.append(-((1 - m) // 2))               # the first x with 2x+1 >= m: ceil((m - 1) / 2)
        hi.append((M - 1) // 2 + 1)              # one past the last x with 2x+1 <= M
    return lo, hi


def clip(lo, hi, dims):
    """[lo, hi) cut to the volume -> (lo, size), or None when nothing is left"""
    l = [max(0, lo[a]) for a in range(3)]
    h = [min(int(dims[a]), hi[a]) for a in range(3)]
    if any(h[a] <= l[a] for a in range(3)):
        return None
    return l, [h[a] - l[a] for a in range(3)]


def inside_mask(shape, p, dims, everywhere=False):
    """bool [z, y, x]: the voxels of a W x H x D volume the shape covers.  The predicate is evaluated over the shape's bounds grown
    by two voxels (everywhere: over the whole volume), in Python integers."""
    W, H, D = (int(v) for v in dims)
    mask = np.zeros((D, H, W), bool)
    lo, hi = bounds(shape, p)
    box = clip([0, 0, 0], [W, H, D], dims) if everywhere else clip([v - 2 for v in lo], [v + 2 for v in hi], dims)
    if box is None:
        return mask
    (x0, y0, z0), (nx, ny, nz) = box
    z, y, x = np.meshgrid(np.arange(z0, z0 + nz), np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij")
    mask[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = inside(shape, p, x.astype(object), y.astype(object), z.astype(object))
    return mask


def value(mode, old, vid, match):
    """what voxels inside the shape become (old: uint8 array)"""
    old = np.asarray(old, np.uint8)
    new = np.uint8(vid)
    if mode == SET:
        return np.full_like(old, new)
    if mode == PAINT:
        return np.where(old != 0, new, old)
    if mode == ADD:
        return np.where(old == 0, new, old)
    assert mode == REPLACE
    return np.where(old == np.uint8(match), new, old)


def tight(before, after):
    """(changed, lo, size) of two volumes: how many voxels differ and their tight box, zeros when none does"""
    diff = before != after
    n = int(diff.sum())
    if n == 0:
        return 0, [0, 0, 0], [0, 0, 0]
    zs, ys, xs = np.nonzero(diff)
    lo = [int(xs.min()), int(ys.min()), int(zs.min())]
    return n, lo, [int(xs.max()) - lo[0] + 1, int(ys.max()) - lo[1] + 1, int(zs.max()) - lo[2] + 1]


def brush(vol, shape, mode, p, vid=0, match=0, everywhere=False):
    """-> (the volume after the brush, (changed, lo, size)); vol itself is left alone"""
    assert shape_ok(shape, p) and mode_ok(mode, vid, match)
    D, H, W = vol.shape
    m = inside_mask(shape, p, (W, H, D), everywhere)
    out = vol.copy()
    out[m] = value(mode, vol[m], vid, match)
    return out, tight(vol, out)


# ---- stamps ---------------------------------------------------------------------------------------------------------------------
def orient_ok(orient):
    return 0 <= orient < 64 and (orient & 7) < 6


def stamp_dst_size(orient, size):
    return [int(size[PERMS[orient & 7][a]]) for a in range(3)]


def stamp_source(orient, size, d):
    """destination offset d = (dx, dy, dz) inside the oriented box -> the source offset"""
    s = [0, 0, 0]
    for a in range(3):
        t = PERMS[orient & 7][a]
        s[t] = int(size[t]) - 1 - int(d[a]) if (orient >> (3 + a)) & 1 else int(d[a])
    return s


def oriented(box, orient):
    """a source box [z, y, x] as the stamp lays it down, [z, y, x] of stamp_dst_size -- by numpy's transpose and flip, which
    test_brush_cpu.py holds against stamp_source voxel by voxel"""
    perm = PERMS[orient & 7]
    out = np.transpose(box, tuple(2 - perm[2 - k] for k in range(3)))          # array axis k is coordinate axis 2 - k
    for a in range(3):
        if (orient >> (3 + a)) & 1:
            out = np.flip(out, axis=2 - a)
    return out


def stamp(dst, dst_lo, src, src_lo, size, orient=0, skip_empty=False):
    """-> (dst after the stamp, (changed, lo, size)); the source box is read before anything is written"""
    assert orient_ok(orient) and all(1 <= int(s) <= STAMP_MAX_SIDE for s in size)
    sx, sy, sz = (int(v) for v in src_lo)
    nx, ny, nz = (int(v) for v in size)
    D, H, W = src.shape
    assert 0 <= sx and sx + nx <= W and 0 <= sy and sy + ny <= H and 0 <= sz and sz + nz <= D
    img = oriented(src[sz:sz + nz, sy:sy + ny, sx:sx + nx].copy(), orient)
    dn = stamp_dst_size(orient, size)
    out = dst.copy()
    D, H, W = dst.shape
    box = clip([int(v) for v in dst_lo], [int(dst_lo[a]) + dn[a] for a in range(3)], (W, H, D))
    if box is not None:
        (x0, y0, z0), (cx, cy, cz) = box
        ox, oy, oz = x0 - int(dst_lo[0]), y0 - int(dst_lo[1]), z0 - int(dst_lo[2])
        part = img[oz:oz + cz, oy:oy + cy, ox:ox + cx]
        old = dst[z0:z0 + cz, y0:y0 + cy, x0:x0 + cx]
        out[z0:z0 + cz, y0:y0 + cy, x0:x0 + cx] = np.where(part == 0, old, part) if skip_empty else part
    return out, tight(dst, out)
