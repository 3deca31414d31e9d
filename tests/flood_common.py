"""What the CPU and GPU tests of vrt_scene_flood share: the small volumes built to break a tiled flood (a plus through every face
of a tile, blocks in diagonal contact, a maze inside one tile, a serpentine across tile planes, a leaking cavity), the thinning
of a volume to a percolation threshold, and the seeded flood sequence.  Volumes are uint8 arrays indexed [z, y, x]."""
import numpy as np

import flood_reference as F

P6, P26 = 0.31, 0.10            # site-percolation thresholds of the cubic lattice, about: 6- and 26-connectivity


def plus_volume():
    """24^3, one plus-shaped object centred in the middle tile: it leaves that tile through each of its six faces"""
    vol = np.zeros((24, 24, 24), np.uint8)
    vol[12, 12, 4:20] = 5; vol[12, 4:20, 12] = 5; vol[4:20, 12, 12] = 5
    return vol, (12, 12, 12), 3 * 16 - 2


def diagonal_volume(kind, a):
    """24^3, two 2^3 blocks that touch only along an edge (kind 'edge') or at a corner ('corner'), the contact between voxels
    a - 1 | a: a = 8 lies exactly on a tile edge or corner, a = 12 inside a tile.  -> (volume, a voxel of each block)"""
    vol = np.zeros((24, 24, 24), np.uint8)
    vol[a - 2:a, a - 2:a, a - 2:a] = 4
    z0 = a if kind == "corner" else a - 2
    vol[z0:z0 + 2, a:a + 2, a:a + 2] = 4
    return vol, (a - 1, a - 1, a - 1), (a, a, z0)


def maze_volume(seed):
    """8^3 of id 9 with a corridor of air: a spanning tree of the 4^3 cells at odd coordinates, carved by a seeded depth-first
    walk.  -> (volume, one end of its longest path, the path's length in steps)"""
    rng = np.random.default_rng(seed)
    vol = np.full((8, 8, 8), 9, np.uint8)
    start = (1, 1, 1)
    vol[start[2], start[1], start[0]] = 0
    seen, stack = {start}, [start]
    while stack:
        c = stack[-1]
        nb = [(c[0] + dx, c[1] + dy, c[2] + dz) for dx, dy, dz in ((2, 0, 0), (-2, 0, 0), (0, 2, 0), (0, -2, 0), (0, 0, 2), (0, 0, -2))]
        nb = [n for n in nb if all(1 <= v <= 7 for v in n) and n not in seen]
        if not nb:
            stack.pop()
            continue
        n = nb[int(rng.integers(len(nb)))]
        vol[(c[2] + n[2]) // 2, (c[1] + n[1]) // 2, (c[0] + n[0]) // 2] = 0
        vol[n[2], n[1], n[0]] = 0
        seen.add(n); stack.append(n)

    def farthest(src):
        dist, frontier = {src: 0}, [src]
        while frontier:
            nxt = []
            for c in frontier:
                for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                    n = (c[0] + dx, c[1] + dy, c[2] + dz)
                    if all(0 <= v <= 7 for v in n) and n not in dist and vol[n[2], n[1], n[0]] == 0:
                        dist[n] = dist[c] + 1; nxt.append(n)
            frontier = nxt
        end = max(dist, key=dist.get)
        return end, dist[end]
    end, _ = farthest(start)
    _, steps = farthest(end)
    return vol, end, steps


def serpentine_volume(cut=None):
    """24 x 24 x 8, one snake of id 6 at z = 3: every even row over the full x length, joined to the next at alternating ends.
    It crosses both tile planes in x on every row and re-enters tiles it has left.  cut: a voxel (x, y) taken out.
    -> (volume, its first voxel, its middle voxel, its voxels in order)"""
    vol = np.zeros((8, 24, 24), np.uint8)
    path = []
    for k, y in enumerate(range(0, 24, 2)):
        xs = list(range(24)) if k % 2 == 0 else list(range(23, -1, -1))
        path += [(x, y, 3) for x in xs]
        if y + 2 < 24:
            path.append((xs[-1], y + 1, 3))
    for x, y, z in path:
        vol[z, y, x] = 6
    if cut is not None:
        vol[3, cut[1], cut[0]] = 0
    return vol, path[0], path[len(path) // 2], path


def cavity_volume():
    """40 x 24 x 32: a hollow box of id 8 (walls one voxel thick, outer box (8, 4, 6) + (20, 14, 16)) with one hole in its +x wall
    -> (volume, a voxel inside, the inside's voxel count)"""
    vol = np.zeros((32, 24, 40), np.uint8)
    vol[6:22, 4:18, 8:28] = 8
    vol[7:21, 5:17, 9:27] = 0
    vol[12, 10, 27] = 0                                            # the hole
    return vol, (12, 9, 10), 18 * 12 * 14


def thin(vol, lo, size, p, seed):
    """the sub-box rewritten with seeded random voxels at occupancy p (ids 1..3): ramified clusters near a threshold"""
    rng = np.random.default_rng(seed)
    out = vol.copy()
    sx, sy, sz = (int(v) for v in size)
    out[lo[2]:lo[2] + sz, lo[1]:lo[1] + sy, lo[0]:lo[0] + sx] = ((rng.random((sz, sy, sx)) < p) * rng.integers(1, 4, (sz, sy, sx))).astype(np.uint8)
    return out


def random_volume(dims, p, seed):
    W, H, D = dims
    return thin(np.zeros((D, H, W), np.uint8), (0, 0, 0), dims, p, seed)


def flood_sequence(vol, box_lo, box_size, n, seed):
    """n seeded floods inside and around the thinned sub-box: alternating predicates, connectivities, ids (0 included) and
    bounds (the whole volume, the sub-box, a box that leaves the volume); seeds on solid and on empty voxels"""
    D, H, W = vol.shape
    rng = np.random.default_rng(seed)
    seq = []
    for k in range(n):
        match = F.SAME if k % 2 == 0 else F.SOLID
        conn = F.FACES if (k // 2) % 2 == 0 else F.CORNERS
        vid = [0, 77, 3, 120][k % 4] if k % 5 else 0
        bounds = [None, (tuple(box_lo), tuple(box_size)), ((-3, box_lo[1] - 2, -5), (box_lo[0] + box_size[0] + 1, box_size[1] + 4, box_lo[2] + box_size[2] + 7))][k % 3]
        s = [int(rng.integers(box_lo[a], box_lo[a] + box_size[a])) for a in range(3)]
        seq.append({"seed": tuple(s), "id": vid, "match": match, "conn": conn, "bounds": bounds})
    return seq
