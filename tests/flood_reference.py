"""The definition vrt_scene_flood is held to (csrc/vrt_flood.h): a plain breadth-first search over a numpy volume, in Python
integers.  No tiles, no masks, no rounds: a queue of voxels.  Volumes are uint8 arrays indexed [z, y, x]."""
from collections import deque

import numpy as np

SAME, SOLID = 0, 1
FACES, CORNERS = 6, 26
MATCHES = {"same": SAME, "solid": SOLID}
MEASURE = 1
MAX_SIDE, MAX_SIZE = 512, 1 << 30
ZERO = {"region": 0, "region_lo": (0, 0, 0), "region_size": (0, 0, 0), "seed_id": 0, "changed": 0, "lo": (0, 0, 0), "size": (0, 0, 0)}


def args_ok(match, conn, flags, size):
    return match in (SAME, SOLID) and conn in (FACES, CORNERS) and (flags & ~MEASURE) == 0 and all(1 <= int(s) <= MAX_SIZE for s in size)


def clip(lo, size, dims):
    """[lo, lo + size) cut to the volume -> (lo, size), or None when nothing is left"""
    l = [max(0, int(lo[a])) for a in range(3)]
    h = [min(int(dims[a]), int(lo[a]) + int(size[a])) for a in range(3)]
    if any(h[a] <= l[a] for a in range(3)):
        return None
    return l, [h[a] - l[a] for a in range(3)]


def offsets(conn):
    out = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                n = abs(dx) + abs(dy) + abs(dz)
                if n == 1 or (conn == CORNERS and n > 1):
                    out.append((dx, dy, dz))
    return out


def component(passable, seed, conn):
    """passable: bool [z, y, x]; seed: (x, y, z) inside it -> bool [z, y, x], the component of the seed (empty if the seed does
    not pass).  A queue over a copy of the mask with a border of False, so no neighbour needs a bounds test."""
    D, H, W = passable.shape
    pad = np.zeros((D + 2, H + 2, W + 2), np.uint8)
    pad[1:-1, 1:-1, 1:-1] = passable
    sy, sz = W + 2, (W + 2) * (H + 2)
    left = bytearray(pad.tobytes())                                # passable and not yet reached
    got = bytearray(len(left))
    at = (int(seed[0]) + 1) + (int(seed[1]) + 1) * sy + (int(seed[2]) + 1) * sz
    if left[at]:
        steps = [dx + dy * sy + dz * sz for dx, dy, dz in offsets(conn)]
        left[at] = 0; got[at] = 1
        queue = deque([at])
        while queue:
            i = queue.popleft()
            for d in steps:
                n = i + d
                if left[n]:
                    left[n] = 0; got[n] = 1
                    queue.append(n)
    return np.frombuffer(bytes(got), np.uint8).reshape(D + 2, H + 2, W + 2)[1:-1, 1:-1, 1:-1].astype(bool)


def tight(mask):
    n = int(mask.sum())
    if n == 0:
        return 0, (0, 0, 0), (0, 0, 0)
    zs, ys, xs = np.nonzero(mask)
    lo = (int(xs.min()), int(ys.min()), int(zs.min()))
    return n, lo, (int(xs.max()) - lo[0] + 1, int(ys.max()) - lo[1] + 1, int(zs.max()) - lo[2] + 1)


def flood(vol, seed, vid, match=SAME, conn=FACES, bounds=None, measure=False):
    """-> (the volume after the flood, the result as VoxelScene.flood returns it); vol itself is left alone"""
    D, H, W = vol.shape
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    assert args_ok(match, conn, 0, size)
    box = clip(lo, size, (W, H, D))
    if box is None or any(not box[0][a] <= int(seed[a]) < box[0][a] + box[1][a] for a in range(3)):
        return vol.copy(), dict(ZERO)
    (x0, y0, z0), (nx, ny, nz) = box
    assert max(nx, ny, nz) <= MAX_SIDE
    sub = vol[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]
    seed_id = int(vol[seed[2], seed[1], seed[0]])
    passable = (sub == seed_id) if match == SAME else (sub != 0)
    reg = np.zeros(vol.shape, bool)
    reg[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = component(passable, (seed[0] - x0, seed[1] - y0, seed[2] - z0), conn)
    n, rlo, rsize = tight(reg)
    res = dict(ZERO, region=n, region_lo=rlo, region_size=rsize, seed_id=seed_id)
    out = vol.copy()
    if not measure:
        out[reg] = vid
        res["changed"], res["lo"], res["size"] = tight(out != vol)
    return out, res


def region(vol, seed, match=SAME, conn=FACES, bounds=None):
    r = flood(vol, seed, 0, match, conn, bounds, measure=True)[1]
    return r["region"], r["region_lo"], r["region_size"]
