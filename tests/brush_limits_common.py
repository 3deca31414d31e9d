"""The brushes and stamps of vrt_scene_brush / vrt_scene_stamp at their documented limits, as data: shared by
tests/test_brush_limits_cpu.py (which proves on tests/brush_reference.py alone that the tables reach what they claim) and
tests/test_gpu_brush_limits.py (which runs them on the device).  A brush is brush_common.op's dictionary; a stamp is
{"kind", "stamp": (dst_lo, src_lo, size, orient, skip_empty)} -- of the scene onto itself where no source is named.

  group A  shape parameters at their limits on 70 x 45 x 52 and 72 x 48 x 56: semi-axes of 1024 and 1023 half voxels, capsules from
           -4096 to 12288, boxes of 2^30.  `reach` of a case is floor(log2) of the largest product the predicate forms over the
           voxels of its clipped bounds (the left-hand side of the ellipsoid's test, da2 * L2 of the capsule's third branch):
           written down here, recomputed by the CPU test.
  group B  brushes and self-stamps on 4096 x 8 x 8 and its transposes, dense and as 512 bricks.
  group C  the ids a stamp writes: sources for the set of written ids (BrushRecord::ids) that decides metallic_voxels.
  group D  stamps with a side of 512 and destinations at the int32 edges.

What the limits allow (and what they do not):
  * an ellipsoid's left-hand side is at most 3 rx^2 ry^2 rz^2, so only (1024, 1024, 1024) can reach 2^59; a flat one -- a
    semi-axis of 1 -- stays below 3 * 2^40 wherever it is centred.  Its rim cannot cross the volume along the flat axis from a
    centre outside either (a semi-axis of one half voxel reaches no voxel centre from outside), so a flat ellipsoid has rim cases
    along its two long axes, both directions, and is centred on a voxel centre in the flat one.
  * da2 * L2 reaches 2^57 only from the far end of a diagonal: L2 = 3 * 2^28 and |P - a|^2 = 3 * 12288^2 on the space diagonal
    (2^58.3), 2^29 and 2 * 12288^2 on a face diagonal (2^57.2); a line along one axis stays at 2^55.2.
  * a line through the volume cannot have EVERY end coordinate at -4096 or 12288 unless it is the space diagonal: a coordinate
    both ends share and that is at a limit puts the line 3072 half voxels outside (the radius is at most 1024).  So every
    coordinate in which the ends differ is at the limits, one end each; a shared one lies in the volume, or -- for the radii 1023
    and 1024 -- outside it by so much that the rim crosses the volume."""
import functools

import numpy as np

import brush_common as bc
import brush_reference as R
import extents_common as X

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
CMIN, CMAX, BIG = R.CAPSULE_MIN, R.CAPSULE_MAX, R.BOX_MAX_SIZE
ELLIPSOID_REACH, CAPSULE_REACH = 59, 57        # conditions on the inputs (the header's own bounds: 2^62, 2^60)

A_SCENES = [("dense-70x45x52", bc.DENSE_A, False), ("bricks-9x6x7", bc.BRICKS, True)]


def a_volume(dims, bricks):
    return bc.brick_volume(dims, 7) if bricks else bc.dense_volume(dims, sum(dims))


def all_bricks_spare(vol):
    """free slots for every brick that is empty: no brush of these tables is refused for want of one"""
    return int((~bc.brick_occupancy(vol)).sum())


def case(kind, shape, mode, p, vid=0, match=0, noop=False, rim=False, reach=None):
    o = bc.op(("no-op: " if noop else "") + kind, shape, mode, p, vid, match)
    o.update(rim=rim, reach=reach)
    return o


# ---- group A ------------------------------------------------------------------------------------------------------------------------
RADII = [(1024, 1024, 1024), (1023, 1024, 1), (1, 1023, 1024), (1024, 1, 1023)]
# reach per semi-axes: a rim case of the sphere 2^60 (a voxel beyond the rim: |d|^2 > 2^20 times 2^40); the flat ones 2^40
RADII_REACH = {RADII[0]: 60, RADII[1]: 40, RADII[2]: 40, RADII[3]: 40}


def ellipsoid_cases(dims):
    """{group: cases}.  A rim case of the sphere: the centre outside the volume along axis a, the rim (centre -+ r_a) in the middle
    of the volume, the centre of the middle voxel on the other axes.  A rim case of a flat ellipsoid: the centre outside along
    both long axes, 0.8 r_a and 0.6 r_b from the middle, so that the rim crosses the middle of the volume obliquely (0.8^2 + 0.6^2
    = 1).  In turn a carve (SET of 0) and a REPLACE of air: what one case empties the next can fill, so every case changes
    something; SET of an id that is not 0 is the groups' last case and the capsules'."""
    groups, vid = {}, 100
    mid = [d | 1 for d in dims]                                    # half voxels: the centre of voxel dims // 2
    for r in RADII:
        cases = []
        long_axes = [a for a in range(3) if r[a] >= 1023]
        for a in long_axes:
            for far in (0, 1):
                c = list(mid)
                if len(long_axes) == 3:
                    c[a] = dims[a] + r[a] if far else dims[a] - r[a]
                else:
                    b = [t for t in long_axes if t != a][0]
                    c[a] += (1 if far else -1) * 2 * (4 * r[a] // 10)
                    c[b] += (1 if far else -1) * 2 * (3 * r[b] // 10)
                    assert c[b] < 0 or c[b] > 2 * dims[b]
                assert c[a] < 0 or c[a] > 2 * dims[a]
                vid += 1
                carve = len(cases) % 2 == 0
                cases.append(case("ellipsoid %s rim %s%s" % (r, "xyz"[a], "+" if far else "-"), R.ELLIPSOID, R.SET if carve else R.REPLACE, c + list(r),
                                  0 if carve else vid, 0, rim=True, reach=RADII_REACH[r]))
        groups["ellipsoid-%dx%dx%d" % r] = cases
    # the whole volume inside: last of its group (the volume is solid afterwards); the farthest voxel is below 2^14 half voxels^2 away
    groups["ellipsoid-1024x1024x1024"].append(case("ellipsoid: the whole volume inside", R.ELLIPSOID, R.SET, mid + [1024] * 3, 99, reach=53))
    return groups


def capsule_cases(dims):
    W, H, D = dims
    mx, my, mz = (d | 1 for d in dims)
    lo, hi = CMIN, CMAX
    C, S, A, RP = R.CAPSULE, R.SET, R.ADD, R.REPLACE
    diagonals = [
        case("space diagonal, r 1", C, S, [lo, lo, lo, hi, hi, hi, 1], 121, reach=55),
        case("space diagonal reversed, r 3", C, A, [hi, hi, hi, lo, lo, lo, 3], 122, reach=58),
        case("face diagonal xy, r 3", C, S, [lo, lo, mz, hi, hi, mz, 3], 123, reach=54),
        case("face diagonal xz reversed, r 1", C, A, [hi, my, hi, lo, my, lo, 1], 124, reach=57),
        case("face diagonal xy below the volume, r 1023", C, S, [lo, lo, -1000, hi, hi, -1000, 1023], 125, rim=True, reach=54),
        case("face diagonal yz reversed beside the volume, r 1024", C, RP, [2 * W + 1001, hi, hi, 2 * W + 1001, lo, lo, 1024], 126, 0, rim=True, reach=57),
        case("space diagonal, r 1023: the whole volume", C, RP, [lo, lo, lo, hi, hi, hi, 1023], 127, 0, reach=55),
        case("space diagonal reversed, r 1024: the whole volume", C, S, [hi, hi, hi, lo, lo, lo, 1024], 128, reach=58),
    ]
    axes = [
        case("along x, r 1", C, S, [lo, my, mz, hi, my, mz, 1], 131, reach=52),
        case("along y, r 3", C, A, [mx, lo, mz, mx, hi, mz, 3], 132, reach=52),
        case("along z reversed, r 3", C, S, [mx, my, hi, mx, my, lo, 3], 133, reach=55),
        case("along x beside the volume, r 1023", C, S, [lo, -1003, mz, hi, -1003, mz, 1023], 134, rim=True, reach=52),
        case("along y behind the volume, r 1024", C, RP, [mx, lo, 2 * D + 1000, mx, hi, 2 * D + 1000, 1024], 135, 0, rim=True, reach=52),
        case("along z reversed past the volume's edge, r 1023", C, S, [-700, -700, hi, -700, -700, lo, 1023], 136, rim=True, reach=55),
    ]
    ends = [
        case("a inside the volume, r 3", C, S, [41, 37, 45, hi, hi, hi, 3], 141, reach=42),
        case("b inside the volume, r 3", C, S, [lo, lo, lo, 61, 51, 40, 3], 142, reach=51),
        case("a == b at 12288, r 1024", C, S, [hi] * 6 + [1024], 143, noop=True),
        case("a == b at -4096, r 1", C, S, [lo] * 6 + [1], 144, noop=True),
    ]
    return {"capsule-diagonals": diagonals, "capsule-axes": axes, "capsule-ends": ends}


def box_cases(dims):
    B, S = R.BOX, R.SET
    near = -BIG + 3                                               # the box ends three voxels into the volume
    return {"boxes": [
        case("box lo -2^31", B, S, [INT32_MIN] * 3 + [BIG] * 3, 151, noop=True),
        case("box lo -2^30", B, S, [-BIG] * 3 + [BIG] * 3, 152, noop=True),
        case("box lo -2^30 + 3: three voxels of every axis", B, S, [near] * 3 + [BIG] * 3, 153),
        case("box lo 2^31 - 1", B, S, [INT32_MAX] * 3 + [BIG] * 3, 154, noop=True),
        case("three voxels of x, the volume in y and z", B, R.ADD, [near, 0, 0] + [BIG] * 3, 155),
        case("the volume in x, three voxels of y and z", B, S, [0, near, near] + [BIG] * 3, 156),
        case("three voxels of z, an absent id replaced", B, R.REPLACE, [0, 0, near] + [BIG] * 3, 157, bc.ABSENT_ID, noop=True),
        case("z at 2^31 - 1", B, S, [0, 0, INT32_MAX] + [BIG] * 3, 158, noop=True),
        case("x at -2^31", B, S, [INT32_MIN, 0, 0] + [BIG] * 3, 159, noop=True),
        case("y at -2^30", B, S, [0, -BIG, 0] + [BIG] * 3, 160, noop=True),
        case("box lo 0: the whole volume painted", B, R.PAINT, [0] * 3 + [BIG] * 3, 161),
        case("box lo 0: the block replaced", B, R.REPLACE, [0] * 3 + [BIG] * 3, 162, 161),
    ]}


def group_a(dims):
    g = {}
    g.update(ellipsoid_cases(dims)); g.update(capsule_cases(dims)); g.update(box_cases(dims))
    return g


A_GROUPS = sorted(group_a(bc.DENSE_A))


# ---- group B ------------------------------------------------------------------------------------------------------------------------
B_SCENES = [(tuple(8 * n for n in nb), bricks) for bricks in (False, True) for nb in X.BRICK_NEEDLES]
B_RES = X.FRAMES[1]


def b_volume(dims):
    return X.needle_volume(dims)                                 # (extents_common's brick needle: caps at both ends, one metallic corner)


def limit_ops(dims):
    """the brushes and self-stamps of one 4096-long scene, in order; the same list on the dense and on the brick scene"""
    a = X.long_axis(dims)
    L = dims[a]
    mid = [d // 2 for d in dims]

    def along(v, rest):
        p = list(rest); p[a] = v
        return p
    centre = [2 * t + 1 for t in mid]
    one = lambda x: along(2 * x + 1, centre) + [1, 1, 1]
    rr = along(1024, [5, 7, 5])
    slab = lambda x0, n: along(x0, [0, 0, 0]) + along(n, list(dims))
    E, C, B = R.ELLIPSOID, R.CAPSULE, R.BOX
    return [
        case("semi-axis 1024 on the far face", E, R.SET, along(2 * L, centre) + rr, 65),
        case("one voxel at 4095", E, R.SET, one(L - 1), 64),
        case("one voxel at 4095, carved", E, R.SET, one(L - 1), 0),
        case("one voxel at 0, carved", E, R.SET, one(0), 0),
        case("capsule along the whole axis", C, R.ADD, along(CMIN, centre) + along(CMAX, centre) + [3], 66),
        case("replace what ADD wrote", B, R.REPLACE, [0, 0, 0] + list(dims), 67, 66),
        case("carve brick 511 away", B, R.SET, slab(L - 8, 8), 0),
        case("carve brick 0 away", B, R.SET, slab(0, 8), 0),
        case("ADD makes bricks 0 and 511 appear", C, R.ADD, along(CMAX, centre) + along(CMIN, centre) + [1], 68),
        {"kind": "3584..4095 onto 0..511, the long axis flipped", "stamp": (along(0, [0, 0, 0]), along(L - 512, [0, 0, 0]), along(512, list(dims)), (1 << a) << 3, False)},
        {"kind": "0..511 to 4095 - 255, clipped at the far face", "stamp": (along(L - 1 - 255, [0, 0, 0]), along(0, [0, 0, 0]), along(512, list(dims)), 0, True)},
    ]


# ---- group C ------------------------------------------------------------------------------------------------------------------------
ALL_IDS_DIMS = (17, 5, 3)                                       # 255 voxels
ONE_ID = (200, 223, 224, 255)
SLAB_DIMS = (20, 12, 4)
NEIGHBOURS = (30, 33, 62, 65, 222, 225)                         # metallic in the palette of the word-boundary cases
BOUNDARY_PAIRS = ((31, 32), (63, 64), (223, 224))
FILL_ID = 50


def all_ids_source():
    """every id 1 .. 255 exactly once, in an order that is no ramp"""
    ids = (np.arange(255) * 37 % 255 + 1).astype(np.uint8)
    assert sorted(ids.tolist()) == list(range(1, 256))
    W, H, D = ALL_IDS_DIMS
    return ids.reshape(D, H, W)


def slab_source(vid):
    """empty but for a slab two voxels thick, at the source's low z"""
    W, H, D = SLAB_DIMS
    v = np.zeros((D, H, W), np.uint8)
    v[:2] = vid
    return v


def pair_source(pair):
    W, H, D = SLAB_DIMS
    v = np.zeros((D, H, W), np.uint8)
    v[:2, :, ::2] = pair[0]; v[:2, :, 1::2] = pair[1]
    return v


def one_lane_source(lane_x):
    """66 x 6 x 2 of a non-metallic id but for one voxel of id 255, at x = lane_x of the front slice"""
    v = np.full((2, 6, 66), FILL_ID, np.uint8)
    v[0, 3, lane_x] = 255
    return v


def face_lo(dims, size):
    """dst_lo that centres a box of `size` on the z = 0 face, which frame_setup's camera looks at"""
    return ((dims[0] - size[0]) // 2, (dims[1] - size[1]) // 2, 0)


# ---- group D ------------------------------------------------------------------------------------------------------------------------
LONG = R.STAMP_MAX_SIDE
SIDES = (3, 2)                                                   # the two short sides, in axis order after the long one is taken out


def long_size(s):
    """the source box whose side along axis s is 512: 512 x 3 x 2, 3 x 512 x 2, 2 x 3 x 512"""
    return {0: (LONG, 3, 2), 1: (3, LONG, 2), 2: (2, 3, LONG)}[s]


def long_source(s, bricks):
    """(volume [z, y, x], src_lo): the box long_size(s) inside a scene a little larger; half full, ids 1 .. 198"""
    size = long_size(s)
    lo = (3, 2, 1) if bricks else (1, 1, 1)
    dims = [size[a] + lo[a] + 1 for a in range(3)]
    if bricks:
        dims = [-(-d // 8) * 8 for d in dims]
    rng = np.random.default_rng(100 + s)
    W, H, D = dims
    return ((rng.random((D, H, W)) < 0.5) * rng.integers(1, 199, (D, H, W))).astype(np.uint8), lo


def long_dst_dims(t, bricks):
    """a destination 520 long on axis t"""
    d = [16, 16, 16] if bricks else [9, 11, 9]
    d[t] = 520
    return tuple(d)


def long_stamps(s, t, dims):
    """the stamps of a source long on axis s into the destination long on axis t: each permutation that lays the long side along
    t, plain and with t flipped; with the first of them one slice at either end, and the three wholly outside"""
    perms = [k for k in range(6) if R.PERMS[k][t] == s]
    assert len(perms) == 2 and (0 in perms) == (s == t)
    out = []
    for n, perm in enumerate(perms):
        for flip in (0, 1):
            orient = perm | ((flip << t) | (n << ((t + 1) % 3))) << 3
            dlo = [1 + n, 2 - n, 1]; dlo[t] = 3 + 2 * flip
            out.append(("perm %d flips %d" % (perm, orient >> 3), tuple(dlo), orient, bool(flip), False))
    orient = perms[-1] | (1 << t) << 3
    for kind, v, noop in (("one slice", -(LONG - 1), False), ("far face", dims[t] - 1, False), ("outside", -LONG, True), ("INT32_MIN", INT32_MIN, True), ("INT32_MAX", INT32_MAX, True)):
        dlo = [1, 1, 1]; dlo[t] = v
        out.append((kind, tuple(dlo), orient, False, noop))
    return out


LARGE_DIMS = (520, 518, 3)
LARGE_STAMP = ((5, 3, 1), (0, 0, 0), (LONG, LONG, 2), 2, False)     # x and y exchanged, onto itself, overlapping


def large_volume():
    W, H, D = LARGE_DIMS
    rng = np.random.default_rng(77)
    return ((rng.random((D, H, W)) < 0.3) * rng.integers(1, 199, (D, H, W))).astype(np.uint8)


# ---- the reference side ---------------------------------------------------------------------------------------------------------------
def apply(vol, o, src=None):
    """-> (the volume after, (changed, lo, size)) by tests/brush_reference.py; a brush is evaluated over its clipped bounds grown by
    two voxels (brush_reference.inside_mask), in Python integers"""
    if "stamp" in o:
        dlo, slo, size, orient, skip = o["stamp"]
        return R.stamp(vol, dlo, vol if src is None else src, slo, size, orient, skip)
    return R.brush(vol, o["shape"], o["mode"], o["p"], o["id"], o["match"])


@functools.lru_cache(maxsize=None)
def a_expected(dims, bricks, group):
    """[(volume after, result)] of a group of group A from the scene's first volume; computed once, never written to"""
    vol = a_volume(dims, bricks)
    out = []
    for o in group_a(dims)[group]:
        vol, res = apply(vol, o)
        vol.setflags(write=False)
        out.append((vol, res))
    return out


@functools.lru_cache(maxsize=None)
def b_expected(dims):
    vol = b_volume(dims)
    out = []
    for o in limit_ops(dims):
        vol, res = apply(vol, o)
        vol.setflags(write=False)
        out.append((vol, res))
    return out


def products(o, dims):
    """over the voxels of the clipped bounds, in Python integers: (largest product, {(branch, inside)}, inside anywhere, outside
    anywhere).  The product is the ellipsoid's left-hand side, or da2 * L2 over the voxels of a capsule's third branch (0 where
    none takes it); branch is 0 for everything but a capsule, whose branches are 1 (q <= 0 or L2 == 0), 2 (q >= L2) and 3."""
    lo, hi = R.bounds(o["shape"], o["p"])
    box = R.clip(lo, hi, dims)
    if box is None:
        return 0, set(), False, False
    (x0, y0, z0), (nx, ny, nz) = box
    z, y, x = (g.astype(object) for g in np.meshgrid(np.arange(z0, z0 + nz), np.arange(y0, y0 + ny), np.arange(x0, x0 + nx), indexing="ij"))
    ins = R.inside(o["shape"], o["p"], x, y, z)
    p = R.params(o["p"])
    P = [2 * x + 1, 2 * y + 1, 2 * z + 1]
    if o["shape"] == R.ELLIPSOID:
        d = [P[a] - p[a] for a in range(3)]
        r2 = [p[3 + a] * p[3 + a] for a in range(3)]
        lhs = d[0] * d[0] * (r2[1] * r2[2]) + d[1] * d[1] * (r2[0] * r2[2]) + d[2] * d[2] * (r2[0] * r2[1])
        return int(lhs.max()), {(0, bool(v)) for v in np.unique(ins)}, bool(ins.any()), bool((~ins).any())
    if o["shape"] == R.CAPSULE:
        e = [p[3 + a] - p[a] for a in range(3)]
        L2 = sum(v * v for v in e)
        da = [P[a] - p[a] for a in range(3)]
        q = da[0] * e[0] + da[1] * e[1] + da[2] * e[2]
        da2 = da[0] * da[0] + da[1] * da[1] + da[2] * da[2]
        branch = np.where((q <= 0).astype(bool) | (L2 == 0), 1, np.where((q >= L2).astype(bool), 2, 3))
        third = branch == 3
        big = int((da2 * L2)[third].max()) if third.any() else 0
        return big, {(int(b), bool(v)) for b, v in zip(branch.ravel(), ins.ravel())}, bool(ins.any()), bool((~ins).any())
    return 0, {(0, True)}, True, False
