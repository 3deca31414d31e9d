"""The definition of vrt_scene_list_faces in numpy and Python integers.  Nothing here is shared with csrc/vrt_faces.h.

Directions d: 0 = -x, 1 = +x, 2 = -y, 3 = +y, 4 = -z, 5 = +z.  Face d of a voxel of the box [lo, lo + size) with id != 0 is exposed
iff the voxel across it is empty: outside the volume is empty, outside the box is read from the volume unless `closed`, under which
it is empty.  Runs lie along y for d < 2 and along x otherwise, join exposed faces of one d and one id, and break where the
box-relative coordinate along the run reaches a multiple of 64.  A record is
    bx | by << 8 | bz << 16 | id << 24 | (length - 1) << 32 | d << 40
of the run's lowest voxel; the records come in ascending d, then ascending order key of that voxel (the run axis fastest).
Volumes are indexed [z][y][x]."""
import numpy as np

STEP = [(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)]
SEGMENT = 64
# the quad of direction d: (the two in-plane axes (run axis, third axis), the corners in units of (length, 1) along them)
QUAD = [((1, 2), ((0, 0), (0, 1), (1, 1), (1, 0))),     # -x: y, z
        ((1, 2), ((0, 0), (1, 0), (1, 1), (0, 1))),     # +x
        ((0, 2), ((0, 0), (1, 0), (1, 1), (0, 1))),     # -y: x, z
        ((0, 2), ((0, 0), (0, 1), (1, 1), (1, 0))),     # +y
        ((0, 1), ((0, 0), (0, 1), (1, 1), (1, 0))),     # -z: x, y
        ((0, 1), ((0, 0), (1, 0), (1, 1), (0, 1)))]     # +z


def _halo(vol, lo, size, closed):
    """the box's ids with one voxel of what counts as its surroundings on every side -> [sz + 2][sy + 2][sx + 2]"""
    x, y, z = (int(t) for t in lo)
    sx, sy, sz = (int(t) for t in size)
    if closed:
        return np.pad(vol[z:z + sz, y:y + sy, x:x + sx], 1)
    return np.pad(vol, 1)[z:z + sz + 2, y:y + sy + 2, x:x + sx + 2]


def exposed(vol, lo, size, closed=False):
    """-> (ids of the box [z][y][x], bool [6][z][y][x])"""
    h = _halo(np.asarray(vol, np.uint8), lo, size, closed)
    core = h[1:-1, 1:-1, 1:-1]
    sz, sy, sx = core.shape
    out = np.zeros((6, sz, sy, sx), bool)
    for d, (dx, dy, dz) in enumerate(STEP):
        across = h[1 + dz:1 + dz + sz, 1 + dy:1 + dy + sy, 1 + dx:1 + dx + sx]
        out[d] = (core != 0) & (across == 0)
    return core, out


def pack(bx, by, bz, vid, length, d):
    return (np.asarray(bx, np.uint64) | np.asarray(by, np.uint64) << np.uint64(8) | np.asarray(bz, np.uint64) << np.uint64(16) |
            np.asarray(vid, np.uint64) << np.uint64(24) | (np.asarray(length, np.uint64) - np.uint64(1)) << np.uint64(32) | np.uint64(d) << np.uint64(40))


def unpack(records):
    """-> bx, by, bz, id, length, d as int64 arrays"""
    r = np.asarray(records, np.uint64).reshape(-1)
    f = lambda sh, bits: ((r >> np.uint64(sh)) & np.uint64((1 << bits) - 1)).astype(np.int64)
    return f(0, 8), f(8, 8), f(16, 8), f(24, 8), f(32, 6) + 1, f(40, 3)


def faces(vol, lo, size, runs=True, closed=False):
    """-> (records uint64, counts uint64 (6,)) by array operations"""
    core, exp = exposed(vol, lo, size, closed)
    sz, sy, sx = core.shape
    bz, by, bx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
    recs, counts = [], []
    for d in range(6):
        # the run axis last: flat order is then the order key
        order = (0, 2, 1) if d < 2 else (0, 1, 2)
        e, ids, X, Y, Z = (a.transpose(order) for a in (exp[d], core, bx, by, bz))
        u = Y if d < 2 else X
        cont = np.zeros_like(e)
        if runs:
            cont[..., 1:] = e[..., 1:] & e[..., :-1] & (ids[..., 1:] == ids[..., :-1]) & (u[..., 1:] % SEGMENT != 0)
        e, cont = e.reshape(-1), cont.reshape(-1)
        start = e & ~cont
        group = np.cumsum(start) - 1                      # the run an exposed face belongs to: the latest start at or before it
        length = np.bincount(group[e], minlength=int(start.sum()))
        s = np.flatnonzero(start)
        recs.append(pack(X.reshape(-1)[s], Y.reshape(-1)[s], Z.reshape(-1)[s], ids.reshape(-1)[s], length, d))
        counts.append(s.size)
    return np.concatenate(recs).astype(np.uint64), np.array(counts, np.uint64)


def faces_loops(vol, lo, size, runs=True, closed=False):
    """the same by plain loops (small boxes)"""
    vol = np.asarray(vol, np.uint8)
    D, H, W = vol.shape
    sx, sy, sz = (int(t) for t in size)

    def voxel(b):
        if closed and not all(0 <= b[a] < (sx, sy, sz)[a] for a in range(3)):
            return 0
        p = [int(lo[a]) + b[a] for a in range(3)]
        if not (0 <= p[0] < W and 0 <= p[1] < H and 0 <= p[2] < D):
            return 0
        return int(vol[p[2], p[1], p[0]])

    def is_exposed(b, d):
        inside = all(0 <= b[a] < (sx, sy, sz)[a] for a in range(3))
        return inside and voxel(b) != 0 and voxel([b[a] + STEP[d][a] for a in range(3)]) == 0

    recs, counts = [], []
    for d in range(6):
        ua = 1 if d < 2 else 0
        n = 0
        keyed = []
        for bz in range(sz):
            for by in range(sy):
                for bx in range(sx):
                    b = [bx, by, bz]
                    if not is_exposed(b, d):
                        continue
                    below = list(b); below[ua] -= 1
                    if runs and b[ua] % SEGMENT != 0 and is_exposed(below, d) and voxel(below) == voxel(b):
                        continue                           # continues a run
                    length = 1
                    nxt = list(b); nxt[ua] += 1
                    while runs and nxt[ua] % SEGMENT != 0 and is_exposed(nxt, d) and voxel(nxt) == voxel(b):
                        length += 1
                        nxt[ua] += 1
                    key = by + (bx + bz * sx) * sy if d < 2 else bx + (by + bz * sy) * sx
                    keyed.append((key, bx | by << 8 | bz << 16 | voxel(b) << 24 | (length - 1) << 32 | d << 40))
                    n += 1
        recs += [r for _, r in sorted(keyed)]
        counts.append(n)
    return np.array(recs, np.uint64), np.array(counts, np.uint64)


def order_keys(records, size):
    bx, by, bz, _, _, d = unpack(records)
    sx, sy = int(size[0]), int(size[1])
    return d, np.where(d < 2, by + (bx + bz * sx) * sy, bx + (by + bz * sy) * sx)


def unit_faces(records, shift=(0, 0, 0)):
    """the records face by face, the coordinates moved by shift -> a sorted int64 array of x | y << 12 | z << 24 | id << 36 | d << 44
    (every face once: a face listed twice shows as a repeated key)"""
    bx, by, bz, vid, length, d = unpack(records)
    first = np.cumsum(length) - length
    k = np.arange(int(length.sum())) - np.repeat(first, length)          # 0 .. length - 1 within each record
    bx, by, bz, vid, d = (np.repeat(a, length) for a in (bx, by, bz, vid, d))
    x = bx + np.where(d >= 2, k, 0) + int(shift[0])
    y = by + np.where(d < 2, k, 0) + int(shift[1])
    z = bz + int(shift[2])
    return np.sort(x | y << 12 | z << 24 | vid << 36 | d << 44)


def quad(record, lo):
    """the four corners of a record's quad in voxels, volume coordinates"""
    bx, by, bz, _, length, d = (int(v[0]) for v in unpack([record]))
    base = [int(lo[0]) + bx, int(lo[1]) + by, int(lo[2]) + bz]
    base[d >> 1] += d & 1
    (ua, wa), corners = QUAD[d]
    out = []
    for cu, cw in corners:
        c = list(base)
        c[ua] += cu * length
        c[wa] += cw
        out.append(tuple(c))
    return out


def mesh(records, lo):
    """-> (vertices int32 (nv, 3) in sixteenths of a voxel, welded in order of first appearance, quads uint32 (n, 4), ids uint8 (n,))"""
    seen, verts, quads = {}, [], []
    for r in records:
        q = []
        for c in quad(r, lo):
            if c not in seen:
                seen[c] = len(verts)
                verts.append([16 * t for t in c])
            q.append(seen[c])
        quads.append(q)
    return (np.array(verts, np.int32).reshape(-1, 3), np.array(quads, np.uint32).reshape(-1, 4), unpack(records)[3].astype(np.uint8))


def triangles(quads):
    q = np.asarray(quads, np.uint32).reshape(-1, 4)
    return np.array([tri for t in q for tri in ((t[0], t[1], t[2]), (t[0], t[2], t[3]))], np.uint32).reshape(-1, 3)
