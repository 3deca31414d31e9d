"""What vrt_scene_components, vrt_scene_component_labels and vrt_scene_filter_components compute, by the definition: a plain
breadth-first search in Python integers over the clipped bounds, then numbering by root.  Independent of csrc/vrt_components.h
(no union-find, no tiles).  Volumes are uint8 arrays indexed [z, y, x]; positions and sizes are (x, y, z)."""
import itertools

import numpy as np

SOLID, SAME, EMPTY = 0, 1, 2
FACES, CORNERS = 6, 26
KEEP_LARGEST, MEASURE = 1, 2
NONE = 0xFFFFFFFF
MATCHES = {"solid": SOLID, "same": SAME, "empty": EMPTY}
MAX_SIDE, MAX_SIZE = 512, 1 << 30

OFFSETS = {FACES: [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)],
           CORNERS: [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]}


def clip(dims, lo, size):
    """-> (clo, csize), or None when nothing is left"""
    clo, cs = [], []
    for a in range(3):
        l, h = max(int(lo[a]), 0), min(int(lo[a]) + int(size[a]), int(dims[a]))
        if h <= l:
            return None
        clo.append(l); cs.append(h - l)
    return tuple(clo), tuple(cs)


def args_ok(match, conn, flags, size):
    return match in (SOLID, SAME, EMPTY) and conn in (FACES, CORNERS) and flags == 0 and all(1 <= int(s) <= MAX_SIZE for s in size)


def filter_ok(min_voxels, max_voxels, faces_all, faces_none, flags):
    return min_voxels <= max_voxels and ((faces_all | faces_none) & ~63) == 0 and (flags & ~3) == 0


def key(match, vid):
    if match == EMPTY:
        return 1 if vid == 0 else 0
    if match == SAME:
        return int(vid)
    return 1 if vid != 0 else 0


def components(vol, match=SOLID, conn=FACES, bounds=None):
    """-> (records, result, labels, (clo, csize)): records a list of dicts in component order, result as VoxelScene.components
    returns it, labels a uint32 array [z, y, x] over the clipped bounds; (None, zeros, None, None) for bounds outside the volume"""
    D, H, W = vol.shape
    match = MATCHES.get(match, match)
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    cl = clip((W, H, D), lo, size)
    if cl is None:
        return [], {"components": 0, "voxels": 0, "largest": 0}, None, None
    clo, cs = cl
    sub = vol[clo[2]:clo[2] + cs[2], clo[1]:clo[1] + cs[1], clo[0]:clo[0] + cs[0]]
    # the keys in a flat list with a border of 0 (does not pass) around the clipped bounds: a neighbour is an index offset
    px, py = cs[0] + 2, cs[1] + 2
    keys = [0] * (px * py * (cs[2] + 2))
    for z in range(cs[2]):
        for y in range(cs[1]):
            row = sub[z, y].tolist()
            at = 1 + (y + 1) * px + (z + 1) * px * py
            keys[at:at + cs[0]] = [key(match, v) for v in row]
    labels = np.full((cs[2], cs[1], cs[0]), NONE, np.uint32)
    records = []
    offs = [dx + dy * px + dz * px * py for dx, dy, dz in OFFSETS[conn]]
    for z in range(cs[2]):                                       # ascending linear index: the first voxel of a component met is its root
        for y in range(cs[1]):
            for x in range(cs[0]):
                start = 1 + x + (y + 1) * px + (z + 1) * px * py
                k = keys[start]
                if k == 0:
                    continue
                n = len(records)
                keys[start] = 0                                  # a voxel met passes no more
                frontier, found = [start], []
                while frontier:
                    nxt = []
                    for c in frontier:
                        found.append(c)
                        for o in offs:
                            if keys[c + o] == k:
                                keys[c + o] = 0
                                nxt.append(c + o)
                    frontier = nxt
                members = [(c % px - 1, c // px % py - 1, c // (px * py) - 1) for c in found]
                mn = [min(m[a] for m in members) for a in range(3)]
                mx = [max(m[a] for m in members) for a in range(3)]
                faces = 0
                for a in range(3):
                    if mn[a] == 0:
                        faces |= 1 << (2 * a)
                    if mx[a] == cs[a] - 1:
                        faces |= 2 << (2 * a)
                for m in members:
                    labels[m[2], m[1], m[0]] = n
                records.append({"root": (clo[0] + x, clo[1] + y, clo[2] + z), "id": int(sub[z, y, x]), "voxels": len(members),
                                "lo": tuple(clo[a] + mn[a] for a in range(3)), "size": tuple(mx[a] - mn[a] + 1 for a in range(3)), "faces": faces})
    largest = 0
    for n, r in enumerate(records):
        if r["voxels"] > records[largest]["voxels"]:
            largest = n
    return records, {"components": len(records), "voxels": sum(r["voxels"] for r in records), "largest": largest}, labels, (clo, cs)


def selected(rec, n, largest, min_voxels, max_voxels, faces_all, faces_none, flags):
    if not min_voxels <= rec["voxels"] <= max_voxels:
        return False
    if (rec["faces"] & faces_all) != faces_all or (rec["faces"] & faces_none) != 0:
        return False
    return not ((flags & KEEP_LARGEST) and n == largest)


ZERO_EDIT = {"changed": 0, "lo": (0, 0, 0), "size": (0, 0, 0)}


def filter_components(vol, vid, match=SOLID, conn=FACES, bounds=None, min_voxels=0, max_voxels=2 ** 64 - 1, faces_all=0, faces_none=0, keep_largest=False,
                      measure=False):
    """-> (the volume after, the result as VoxelScene.filter_components returns it)"""
    flags = (KEEP_LARGEST if keep_largest else 0) | (MEASURE if measure else 0)
    records, result, labels, cl = components(vol, match, conn, bounds)
    out = vol.copy()
    res = {"components": 0, "voxels": 0, **ZERO_EDIT}
    if not records:
        return out, res
    clo, cs = cl
    sel = np.array([selected(r, n, result["largest"], min_voxels, max_voxels, faces_all, faces_none, flags) for n, r in enumerate(records)], bool)
    res["components"] = int(sel.sum())
    res["voxels"] = sum(r["voxels"] for r, s in zip(records, sel) if s)
    if measure:
        return out, res
    inside = np.zeros(labels.shape, bool)
    passing = labels != NONE
    inside[passing] = sel[labels[passing]]
    sub = out[clo[2]:clo[2] + cs[2], clo[1]:clo[1] + cs[1], clo[0]:clo[0] + cs[0]]
    changed = inside & (sub != vid)
    if changed.any():
        zz, yy, xx = np.nonzero(changed)
        mn = (int(xx.min()), int(yy.min()), int(zz.min()))
        mx = (int(xx.max()), int(yy.max()), int(zz.max()))
        res.update(changed=int(changed.sum()), lo=tuple(clo[a] + mn[a] for a in range(3)), size=tuple(mx[a] - mn[a] + 1 for a in range(3)))
        sub[inside] = vid
    return out, res


def records_array(records, dtype):
    """the reference's records as the structured array VoxelScene.components returns"""
    out = np.zeros(len(records), dtype)
    for n, r in enumerate(records):
        out[n]["root"] = r["root"]; out[n]["id"] = r["id"]; out[n]["voxels"] = r["voxels"]
        out[n]["lo"] = r["lo"]; out[n]["size"] = r["size"]; out[n]["faces"] = r["faces"]
    return out
