"""One scene through every rewriting tool in turn: the session as data, and its model.

A session is a list of steps, plain dicts, made from a seed by session(dims, bricks, seed, n_steps).  A REWRITING step calls one
of the eight tools (edit, fill, brush, stamp, flood, morph, filter, voxelize); a READING step asks the scene something and must
leave it alone.  The generator alone decides the steps; what a step does is the references' business: the model is a numpy volume
[z, y, x] advanced by brush_reference, flood_reference, morph_reference, components_reference, voxelize_reference and plain
slicing.  On a brick scene the model also keeps the pool: the rule of brush_common.needs_more_slots decides whether a step is
refused, and Slots restates which slot a brick takes and gives back (csrc/vrt_api_edit.hip, brick_scene_edit): the bricks of the
edited box in index order, those that vanish push their slots, those that appear pop.

tests/test_session_cpu.py proves on the references alone that the table reaches what it claims; tests/test_gpu_session.py holds
the device to it.

The table: three seeds per volume, every session in full (len(session(...)) steps, about 70).
    dense-a  70 x 45 x 52 (brush_common.DENSE_A)   seeds 1, 2, 3
    dense-b  150 x 9 x 11 (brush_common.DENSE_B)   seeds 4, 5, 6
    bricks   72 x 48 x 56 (brush_common.BRICKS, reserved with BRICK_SPARE)   seeds 7, 8, 9
The tool that first writes a metallic id is METAL_TOOLS[seed % 5]: the nine seeds reach all five."""
import functools

import numpy as np

import brush_common as bc
import brush_reference as BR
import components_reference as CR
import faces_reference as FR
import flood_reference as LR
import morph_reference as MR
import scene_read_common as RC
import voxelize_common as vc
import voxelize_reference as VR

VOLUMES = {"dense-a": (bc.DENSE_A, False), "dense-b": (bc.DENSE_B, False), "bricks": (bc.BRICKS, True)}
SEEDS = {"dense-a": (1, 2, 3), "dense-b": (4, 5, 6), "bricks": (7, 8, 9)}
TABLE = [(name, seed) for name in VOLUMES for seed in SEEDS[name]]
CHECK_EVERY = 9                                                 # a check point at every 9th step and at the end: 8 or 9 of them
SHORT = 17                                                      # short_session: every tool once
REWRITING = ("edit", "fill", "brush", "stamp", "flood", "morph", "filter", "voxelize")
READING = ("read", "voxels", "count", "face_count", "faces", "components", "region", "morph_measure", "filter_measure", "trace_rays", "pick", "memory", "trim")
SCRATCH = {"edit": "edit_scratch", "fill": "edit_scratch", "brush": "edit_scratch", "stamp": "edit_scratch", "flood": "flood_scratch", "morph": "morph_scratch",
           "filter": "comp_scratch", "voxelize": "voxelize_scratch"}
METAL_TOOLS = ("fill", "flood", "morph", "filter", "voxelize")   # neither brush nor stamp: their metal is pinned by their own files
WALL_ID = 150
STALE, NO_LABELS = "edited after its latest labelling", "no labelling"
ZERO3 = (0, 0, 0)


def start_volume(name):
    dims, bricks = VOLUMES[name]
    return bc.brick_volume(dims, 7) if bricks else bc.dense_volume(dims, sum(dims))


def second_volume():
    """the small scene stamps are also taken from: 13 x 10 x 9, half full"""
    rng = np.random.default_rng(77)
    return ((rng.random((9, 10, 13)) < 0.5) * rng.integers(1, 199, (9, 10, 13))).astype(np.uint8)


def is_large(dims, size):
    return all(4 * int(size[a]) >= 3 * dims[a] for a in range(3))


def is_small(lo, size):
    """inside one 8^3 tile and off its grid"""
    return all(int(lo[a]) % 8 != 0 and int(lo[a]) % 8 + int(size[a]) < 8 for a in range(3))


# ---- the generator ----------------------------------------------------------------------------------------------------------------
def session(dims, bricks, seed, n_steps=None):
    """the steps of one session; n_steps: a prefix (to shrink a failing session by hand)"""
    W, H, D = dims
    rng = np.random.default_rng([int(seed), W, H, D, int(bricks)])
    thin = min(H, D) < 40
    S = []

    def ri(lo, hi):
        return int(rng.integers(lo, hi))

    def add(tool, kind, **a):
        S.append(dict(tool=tool, kind=kind, **a))

    def large():
        lo = [ri(0, min(dims[a] // 8, 3) + 1) for a in range(3)]
        hi = [ri(0, min(dims[a] // 8, 3) + 1) for a in range(3)]
        return lo, [dims[a] - lo[a] - hi[a] for a in range(3)]

    def small():
        t = [ri(0, dims[a] // 8) for a in range(3)]
        off = [ri(1, 4) for _ in range(3)]
        return [8 * t[a] + off[a] for a in range(3)], [ri(3, 8 - off[a]) for a in range(3)]

    def medium():
        """off the grid, a few tiles, inside the volume"""
        size = [max(3, min(dims[a] - 4, ri(11, 22))) for a in range(3)]
        lo = [ri(1, dims[a] - size[a]) for a in range(3)]
        return [v + (v % 8 == 0) for v in lo], [size[a] - 1 for a in range(3)]

    def at(m=5):
        lo = [min(m, (dims[a] - 1) // 2) for a in range(3)]
        return [ri(lo[a], max(lo[a] + 1, dims[a] - m)) for a in range(3)]

    def room(c, r=(3, 2, 2)):
        lo = [max(0, c[a] - r[a]) for a in range(3)]
        return lo, [min(dims[a], c[a] + r[a] + 1) - lo[a] for a in range(3)]

    def random_ids(lo, size):
        shape = (size[2], size[1], size[0])
        ids = ((rng.random(shape) < (0.05 if bricks else 0.03)) * rng.integers(1, 199, shape)).astype(np.uint8)
        if bricks:                                               # a fifth of the bricks hold anything: fewer than in brick_volume, so slots come free
            keep = rng.random((D // 8, H // 8, W // 8)) < 0.2
            z, y, x = ((lo[a] + np.arange(size[a])) // 8 for a in (2, 1, 0))
            ids *= keep[np.ix_(z, y, x)].astype(np.uint8)
        return ids.tolist()

    def mesh(m):
        return {"vertices": np.asarray(m[0]).tolist(), "triangles": np.asarray(m[1]).tolist()}

    def orient():
        return BR.ORIENTS[ri(0, 48)]

    centre = [W // 2, H // 2, D // 2]
    ball_r = 3 if thin else 12
    whole = ([0, 0, 0], [W, H, D])
    metal_tool = METAL_TOOLS[int(seed) % 5]

    add("memory", "memory before the first tool")
    add("brush", "replace the block: large bounds, a small change", shape=BR.BOX, mode=BR.REPLACE, p=[0, 0, 0, W, H, D], id=41, match=bc.BLOCK_ID)
    lo, size = medium()
    add("read", "read a box", lo=lo, size=size)
    lo, size = large()
    add("edit", "edit: a large box of random ids", lo=lo, ids=random_ids(lo, size), extent=(lo, size))
    lo, size = medium()
    add("voxels", "list a box", lo=lo, size=size)
    add("morph", "close r1 /6, whole volume", op=MR.CLOSE, r=1, conn=6, id=90, bounds=None, border=False, extent=whole)
    b = large()
    add("components", "label large bounds, solid /6", match=CR.SOLID, conn=6, bounds=b)
    c1 = at()
    lo, size = room(c1)
    add("fill", "fill a room", lo=lo, size=size, id=61)
    b = large()
    add("flood", "flood solid /26 in large bounds", seed=c1, id=62, match=LR.SOLID, conn=26, bounds=b, extent=b)
    add("region", "measure the region at the room", seed=c1, match=LR.SAME, conn=6, bounds=None)
    b = large()
    add("voxelize", "a closed sphere, surface and solid, set, large bounds", id=81, mode=VR.SET, fill=VR.SURFACE | VR.SOLID, bounds=b, match=0, extent=b,
        **mesh(vc.sphere_mesh([centre[0] + 0.3, centre[1] + 0.2, centre[2] + 0.4], ball_r)))
    lo, size = medium()
    add("faces", "faces of a box in runs", lo=lo, size=size, runs=True, closed=False)
    b = large()
    add("filter", "despeckle /26 in large bounds", id=0, match=CR.SOLID, conn=26, bounds=b, kw={"max_voxels": 1}, extent=b)
    add("trace_rays", "twenty rays", rays=ri(0, 1 << 30))
    # every tool again inside one tile
    sb = small()
    slo, ssz = sb
    add("brush", "set a small box", shape=BR.BOX, mode=BR.SET, p=slo + ssz, id=23, match=0, extent=sb)
    add("flood", "flood same /6 in small bounds", seed=slo, id=24, match=LR.SAME, conn=6, bounds=sb, extent=sb)
    add("morph", "hollow r1 /26 in small bounds", op=MR.HOLLOW, r=1, conn=26, id=0, bounds=sb, border=False, extent=sb)
    tri = [[16 * slo[0] + 2, 16 * slo[1] + 2, 16 * slo[2] + 2], [16 * (slo[0] + ssz[0]) - 2, 16 * (slo[1] + ssz[1]) - 3, 16 * (slo[2] + ssz[2]) - 2],
           [16 * slo[0] + 3, 16 * (slo[1] + ssz[1]) - 2, 16 * slo[2] + 8 * ssz[2]]]
    add("voxelize", "one triangle, surface, add, small bounds", id=26, mode=VR.ADD, fill=VR.SURFACE, bounds=sb, match=0, extent=sb, vertices=tri, triangles=[[0, 1, 2]])
    add("filter", "recolour same /6 in small bounds", id=27, match=CR.SAME, conn=6, bounds=sb, kw={"min_voxels": 1}, extent=sb)
    add("components", "label small bounds, same /26", match=CR.SAME, conn=26, bounds=sb)
    add("memory", "memory with every scratch taken")
    add("trim", "trim")
    add("morph", "erode r1 /6, border solid, whole volume", op=MR.ERODE, r=1, conn=6, id=0, bounds=None, border=True, extent=whole)
    lo, size = medium()
    add("count", "count a box", lo=lo, size=size)
    ec = [20.5, 16.0, 16.5] if not thin else [20.5, 4.0, 5.5]
    add("brush", "add that makes bricks appear", shape=BR.ELLIPSOID, mode=BR.ADD, p=bc.sphere(ec, 9.5 if not thin else 3.5), id=70, match=0)
    b = large()
    add("flood", "flood same /26 in large bounds", seed=[int(v) for v in ec], id=71, match=LR.SAME, conn=26, bounds=b, extent=b)
    add("filter_measure", "measure the small components", id=0, match=CR.SOLID, conn=6, bounds=None, kw={"max_voxels": 5})
    b = large()
    add("filter", "keep the largest /6 in large bounds", id=0, match=CR.SOLID, conn=6, bounds=b, kw={"keep_largest": True}, extent=b)
    b = large()
    blo = [centre[a] - ball_r + 2 for a in range(3)]
    add("voxelize", "a closed box, solid, paint, large bounds", id=82, mode=VR.PAINT, fill=VR.SOLID, bounds=b, match=0, extent=b,
        **mesh(vc.box_mesh([16 * v + 5 for v in blo], [16 * (v + ball_r) + 3 for v in blo])))
    hr = 1 if thin else 8
    b = large()
    add("morph", "hollow /6 in large bounds: a cavity in the ball", op=MR.HOLLOW, r=hr, conn=6, id=0, bounds=b, border=False, extent=b)
    add("pick", "pick the middle pixel")
    b = large()
    add("filter", "fill the cavities /6 in large bounds", id=83, match=CR.EMPTY, conn=6, bounds=b, kw={"faces_none": 63}, extent=b)
    lo, size = large()
    add("edit", "edit: a second large box of random ids", lo=lo, ids=random_ids(lo, size), extent=(lo, size))
    add("morph_measure", "measure a dilation r2 /26", op=MR.DILATE, r=2, conn=26, id=5, bounds=medium(), border=False)
    add("brush", "carve that empties bricks", shape=BR.BOX, mode=BR.SET, p=[6, 5 if not thin else 1, 3 if not thin else 1, 29, 22, 27], id=0, match=0)
    n = [max(3, 3 * dims[a] // 4 if a == 0 or not thin else dims[a] - 2) for a in range(3)]
    add("stamp", "stamp the scene onto itself, overlapping", dst=[3, 1, 1], src="self", src_lo=[0, 0, 0], size=[min(n[0], 60), min(n[1], 30), min(n[2], 30)], orient=0,
        skip_empty=False)
    lo, size = medium()
    add("face_count", "count the faces of a closed box", lo=lo, size=size, runs=False, closed=True)
    ssize = [min(12, dims[0] // 4), min(7, dims[1] // 2), min(9, dims[2] // 2)]
    add("stamp", "stamp a corner far away, oriented, skipping air", dst=[W - ssize[0] - 5, H // 2, D // 2 - 1], src="self", src_lo=[1, 0, 1], size=ssize, orient=orient(),
        skip_empty=True)
    add("stamp", "stamp from a second scene, oriented", dst=[ri(-3, W - 6), ri(-2, H - 3), ri(-2, D - 3)], src="second", src_lo=[1, 1, 0], size=[11, 8, 9], orient=orient(),
        skip_empty=bool(ri(0, 2)))
    b = medium()
    add("morph", "open r2 /26, border solid, off-grid bounds", op=MR.OPEN, r=2, conn=26, id=0, bounds=b, border=True, extent=b)
    b = medium()
    add("components", "label off-grid bounds, same /26", match=CR.SAME, conn=26, bounds=b)
    b = medium()
    add("morph", "dilate r3 /6, off-grid bounds", op=MR.DILATE, r=3, conn=6, id=91, bounds=b, border=False, extent=b)
    lo, size = small() if bricks else medium()
    add("morph", "dilate r8 /26, border solid", op=MR.DILATE, r=8, conn=26, id=92, bounds=(lo, size), border=True, extent=(lo, size))
    c = at()
    add("brush", "capsule, paint", shape=BR.CAPSULE, mode=BR.PAINT, p=[2 * c[0], 2 * c[1] + 1, 2 * c[2], 2 * centre[0] + 1, 2 * centre[1], 2 * centre[2], 5], id=30, match=0)
    c = at()
    add("brush", "ellipsoid, set", shape=BR.ELLIPSOID, mode=BR.SET, p=[2 * c[0] + 1, 2 * c[1], 2 * c[2] + 1, 11, 6, 8], id=31, match=0)
    c = at()
    add("flood", "flood solid /6 in off-grid bounds", seed=c, id=32, match=LR.SOLID, conn=6, bounds=room(c, (9, 4, 4)))
    add("region", "measure a region /26", seed=c, match=LR.SOLID, conn=26, bounds=room(c, (9, 4, 4)))
    c = at()
    add("voxelize", "a tetrahedron, solid, add", id=84, mode=VR.ADD, fill=VR.SOLID, bounds=None, match=0,
        **mesh(vc.tetra_mesh([[16 * c[0] - 40, 16 * c[1] - 30, 16 * c[2] - 33], [16 * c[0] + 45, 16 * c[1] - 20, 16 * c[2] - 25], [16 * c[0] + 3, 16 * c[1] + 41, 16 * c[2] - 19],
                              [16 * c[0] + 7, 16 * c[1] + 2, 16 * c[2] + 47]])))
    add("voxelize", "a few single triangles, surface, paint", id=85, mode=VR.PAINT, fill=VR.SURFACE, bounds=None, match=0, **mesh(vc.tiny_triangles(12, dims, ri(0, 1000))))
    # the first metallic id, written by a tool that is neither brush nor stamp, into a wall that faces the camera
    wall = ([W // 4, 0, 1], [W // 2, H, 2])
    add("fill", "a wall that faces the camera", lo=wall[0], size=wall[1], id=WALL_ID)
    mc = [W // 2, H // 2, 1]
    if metal_tool == "fill":
        add("fill", "metal: fill the wall", lo=wall[0], size=wall[1], id=bc.METAL_ID, metal=True)
    elif metal_tool == "flood":
        add("flood", "metal: flood the wall", seed=mc, id=bc.METAL_ID, match=LR.SAME, conn=6, bounds=None, metal=True)
    elif metal_tool == "morph":
        front = ([W // 4, 0, 0], [W // 2, H, 1])
        add("morph", "metal: dilate the wall towards the camera", op=MR.DILATE, r=1, conn=6, id=bc.METAL_ID, bounds=front, border=False, metal=True)
    elif metal_tool == "filter":
        add("filter", "metal: recolour the wall", id=bc.METAL_ID, match=CR.SAME, conn=6, bounds=wall, kw={"min_voxels": 2 * H}, metal=True)
    else:
        add("voxelize", "metal: a box over the wall", id=bc.METAL_ID, mode=VR.SET, fill=VR.SURFACE | VR.SOLID, bounds=wall, match=0, metal=True,
            **mesh(vc.box_mesh([16 * (W // 4) - 8, -8, 8], [16 * (W // 4 + W // 2) + 8, 16 * H + 8, 56])))
    add("trace_rays", "twenty more rays", rays=ri(0, 1 << 30))
    # the no-ops of every tool
    c = at()
    rb = room(c)
    add("fill", "fill a second room", lo=rb[0], size=rb[1], id=64)
    add("components", "label the whole volume, solid /26", match=CR.SOLID, conn=26, bounds=None)
    add("edit", "no-op: edit the ids already there", lo=rb[0], ids=np.full((rb[1][2], rb[1][1], rb[1][0]), 64, np.uint8).tolist(), noop=True)
    add("fill", "no-op: fill the id already there", lo=rb[0], size=rb[1], id=64, noop=True)
    add("brush", "no-op: wholly outside", shape=BR.ELLIPSOID, mode=BR.SET, p=bc.sphere((-20, H / 2.0, D / 2.0), 6.0), id=59, match=0, noop=True)
    add("brush", "no-op: replace an absent id", shape=BR.BOX, mode=BR.REPLACE, p=[0, 0, 0, W, H, D], id=63, match=bc.ABSENT_ID, noop=True)
    add("stamp", "no-op: stamp a box where it lies", dst=[2, 1, 1], src="self", src_lo=[2, 1, 1], size=[min(40, W - 3), H - 2, D - 2], orient=0, skip_empty=False, noop=True)
    add("flood", "no-op: the id already there", seed=c, id=64, match=LR.SAME, conn=6, bounds=None, noop=True)
    c2 = at()
    ra = room(c2, (2, 1, 1))
    add("fill", "carve a third room", lo=ra[0], size=ra[1], id=0)
    add("flood", "no-op: a seed that is air, solid", seed=c2, id=65, match=LR.SOLID, conn=26, bounds=None, noop=True)
    add("morph", "no-op: bounds wholly outside", op=MR.DILATE, r=2, conn=6, id=66, bounds=([W, 0, 0], [9, 9, 9]), border=False, noop=True)
    add("filter", "no-op: nothing is that large", id=67, match=CR.SOLID, conn=6, bounds=medium(), kw={"min_voxels": 10 ** 9}, noop=True)
    add("filter", "no-op: same, the id already there", id=64, match=CR.SAME, conn=6, bounds=rb, kw={}, noop=True)
    add("voxelize", "no-op: a mesh wholly outside", id=68, mode=VR.SET, fill=VR.SURFACE | VR.SOLID, bounds=None, match=0, noop=True,
        **mesh(vc.box_mesh([-400, -300, -200], [-100, -90, -80])))
    add("voxelize", "no-op: replace an absent id", id=69, mode=VR.REPLACE, fill=VR.SURFACE, bounds=None, match=bc.ABSENT_ID, noop=True,
        **mesh(vc.sphere_mesh([centre[0], centre[1], centre[2]], ball_r)))
    add("memory", "memory after the no-ops")
    if bricks:                                                   # refused for lack of slots, by two tools, after slots were freed and taken again
        add("brush", "refused: add into every brick", shape=BR.BOX, mode=BR.ADD, p=[0, 0, 0, W, H, D], id=72, match=0, refuse=True)
        add("flood", "refused: flood the air", seed=c2, id=33, match=LR.SAME, conn=6, bounds=None, refuse=True)
        add("read", "read after the refusals", lo=[0, 0, 0], size=[W, 8, 8])
    add("trim", "trim again")
    sb = small()
    add("fill", "a small fill after the trim", lo=sb[0], size=sb[1], id=73, extent=sb)
    add("faces", "faces of a closed box, unmerged", lo=[1, 1, 1], size=[min(W - 2, 60), H - 2, D - 2], runs=False, closed=True)
    return S if n_steps is None else S[:n_steps]


def short_session(dims, bricks, seed):
    """every tool once, in the order of the long session (of the stamps the one from the second scene, which needs few slots): what
    the stream test and the two interleaved scenes run"""
    seen, out = set(), []
    for s in session(dims, bricks, seed):
        if s["tool"] in REWRITING and s["tool"] not in seen and not s.get("noop") and not s.get("refuse") and s.get("src", "second") == "second":
            seen.add(s["tool"])
            out.append(s)
        elif s["tool"] in ("read", "count", "components", "region", "trim") and ("r", s["tool"]) not in seen:
            seen.add(("r", s["tool"]))
            out.append(s)
    # a second round of the composed tools, in other bounds: what the first round left in the scratch lies under them
    out += [s for s in session(dims, bricks, seed) if s["kind"] in ("set a small box", "flood same /6 in small bounds", "hollow r1 /26 in small bounds",
                                                                      "recolour same /6 in small bounds")]
    return out


# ---- the model --------------------------------------------------------------------------------------------------------------------
def t3(v):
    return tuple(int(t) for t in v)


def brush_result(res):
    return int(res[0]), t3(res[1]), t3(res[2])


def apply(vol, s, second=None):
    """one rewriting step on the model -> (the volume after, the result as the Python API returns it; None for edit and fill)"""
    t = s["tool"]
    if t == "edit":
        ids = np.asarray(s["ids"], np.uint8)
        out = vol.copy()
        lo = s["lo"]
        out[lo[2]:lo[2] + ids.shape[0], lo[1]:lo[1] + ids.shape[1], lo[0]:lo[0] + ids.shape[2]] = ids
        return out, None
    if t == "fill":
        out = vol.copy()
        lo, size = s["lo"], s["size"]
        out[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = s["id"]
        return out, None
    if t == "brush":
        out, res = BR.brush(vol, s["shape"], s["mode"], s["p"], s["id"], s["match"])
        return out, brush_result(res)
    if t == "stamp":
        out, res = BR.stamp(vol, s["dst"], vol if s["src"] == "self" else second, s["src_lo"], s["size"], s["orient"], s["skip_empty"])
        return out, brush_result(res)
    if t == "flood":
        return LR.flood(vol, s["seed"], s["id"], s["match"], s["conn"], s["bounds"])
    if t == "morph":
        return MR.morph(vol, s["op"], s["r"], s["conn"], s["id"], s["bounds"], s["border"])
    if t == "filter":
        return CR.filter_components(vol, s["id"], s["match"], s["conn"], s["bounds"], **s["kw"])
    assert t == "voxelize", t
    return VR.voxelize(vol, np.asarray(s["vertices"], np.int64), np.asarray(s["triangles"], np.int64), s["id"], s["mode"], s["fill"], s["bounds"], s["match"])


def changed_of(s, res, vol, out):
    if s["tool"] in ("edit", "fill"):
        return int((vol != out).sum())
    return res[0] if isinstance(res, tuple) else res["changed"]


def edited_box(s, res):
    """the box the step hands to the edit pass, [lo, hi): the box given (edit, fill) or the tight box of what changes"""
    if s["tool"] == "edit":
        ids = np.asarray(s["ids"], np.uint8)
        return list(s["lo"]), [s["lo"][0] + ids.shape[2], s["lo"][1] + ids.shape[1], s["lo"][2] + ids.shape[0]]
    if s["tool"] == "fill":
        return list(s["lo"]), [s["lo"][a] + s["size"][a] for a in range(3)]
    lo, size = (res[1], res[2]) if isinstance(res, tuple) else (res["lo"], res["size"])
    return list(lo), [lo[a] + size[a] for a in range(3)]


class Slots:
    """the brick pool as brick_scene_edit keeps it: brick (bx, by, bz) -> slot, and the stack of free slots"""
    def __init__(self, slot_of, capacity):
        self.slot_of = dict(slot_of)
        n = len(self.slot_of)
        assert sorted(self.slot_of.values()) == list(range(n))
        self.free = list(range(capacity - 1, n - 1, -1))         # the lowest fresh slot on top
        self.freed_by = {}                                       # slot -> the tool whose step freed it
        self.handed = []                                         # (step, tool that took, tool that had freed) of every slot taken again

    @classmethod
    def in_index_order(cls, vol, spare):
        occ = np.argwhere(bc.brick_occupancy(vol))
        return cls({(int(x), int(y), int(z)): k for k, (z, y, x) in enumerate(occ)}, len(occ) + spare)

    def edit(self, vol, out, lo, hi, tool, k):
        before, after = bc.brick_occupancy(vol), bc.brick_occupancy(out)
        bricks = [(x, y, z) for z in range(lo[2] >> 3, ((hi[2] - 1) >> 3) + 1) for y in range(lo[1] >> 3, ((hi[1] - 1) >> 3) + 1)
                  for x in range(lo[0] >> 3, ((hi[0] - 1) >> 3) + 1)]
        for x, y, z in bricks:
            if before[z, y, x] and not after[z, y, x]:
                slot = self.slot_of.pop((x, y, z))
                self.free.append(slot)
                self.freed_by[slot] = tool
        for x, y, z in bricks:
            if after[z, y, x] and not before[z, y, x]:
                slot = self.free.pop()
                self.slot_of[(x, y, z)] = slot
                if slot in self.freed_by:
                    self.handed.append((k, tool, self.freed_by.pop(slot)))

    def pointers(self, nb):
        """the pointer of every padded grid entry that is a brick of the volume: slot + 1, 0 for an empty brick"""
        out = np.zeros((nb[2], nb[1], nb[0]), np.int64)
        for (x, y, z), slot in self.slot_of.items():
            out[z, y, x] = slot + 1
        return out


def device_pointers(entries, nb):
    """STATE_BENTRY -> the pointers of the volume's bricks, [bz, by, bx]"""
    e = (entries & bc.PTR).astype(np.int64).reshape(nb[2] + 2, nb[1] + 2, nb[0] + 2)
    return e[1:-1, 1:-1, 1:-1]


def run_model(steps, vol, bricks, second=None, slots=None):
    """every step on the model -> (records, the pool's model or None); a record per step: vol (after the step; the same array as before where nothing
    changed), res, changed, refused, touched (the step reached the edit pass: what makes a labelling stale), free (slots after)"""
    out = []
    if bricks and slots is None:
        slots = Slots.in_index_order(vol, bc.BRICK_SPARE)
    for k, s in enumerate(steps):
        rec = {"vol": vol, "res": None, "changed": 0, "refused": False, "touched": False, "free": len(slots.free) if bricks else 0}
        if s["tool"] in REWRITING:
            new, res = apply(vol, s, second)
            changed = changed_of(s, res, vol, new)
            direct = s["tool"] in ("edit", "fill")
            rec["touched"] = direct or changed > 0
            if bricks and rec["touched"] and bc.needs_more_slots(vol, new, len(slots.free)):
                rec["refused"] = True
            else:
                if bricks and rec["touched"]:
                    lo, hi = edited_box(s, res)
                    slots.edit(vol, new, lo, hi, s["tool"], k)
                rec.update(res=res, changed=changed, free=len(slots.free) if bricks else 0)
                if changed:
                    vol = new
                    rec["vol"] = vol
        out.append(rec)
    return out, slots


@functools.lru_cache(maxsize=None)
def table_model(name, seed):
    """(steps, the model's records, the pool's model) of one entry of the table, computed once and left alone"""
    dims, bricks = VOLUMES[name]
    steps = session(dims, bricks, seed)
    recs, slots = run_model(steps, start_volume(name), bricks, second_volume())
    for r in recs:
        r["vol"].setflags(write=False)
    return steps, recs, slots


# ---- what a reading step answers, on the model ---------------------------------------------------------------------------------
def read_expected(vol, s):
    """the answer of a reading step that needs neither a device nor the oracle"""
    t = s["tool"]
    if t == "read":
        return RC.box_slice(vol, s["lo"], s["size"])
    if t == "voxels":
        return RC.records_of(vol, s["lo"], s["size"])
    if t == "count":
        return int((RC.box_slice(vol, s["lo"], s["size"]) != 0).sum())
    if t == "face_count":
        return FR.faces(vol, s["lo"], s["size"], s["runs"], s["closed"])[1]
    if t == "faces":
        return FR.faces(vol, s["lo"], s["size"], s["runs"], s["closed"])
    if t == "components":
        return CR.components(vol, s["match"], s["conn"], s["bounds"])
    if t == "region":
        return LR.region(vol, s["seed"], s["match"], s["conn"], s["bounds"])
    if t == "morph_measure":
        return MR.morph(vol, s["op"], s["r"], s["conn"], s["id"], s["bounds"], s["border"], measure=True)[1]
    if t == "filter_measure":
        return CR.filter_components(vol, s["id"], s["match"], s["conn"], s["bounds"], measure=True, **s["kw"])[1]
    return None


# ---- the same steps on a scene -----------------------------------------------------------------------------------------------------
def run(sc, s, second=None):
    """one rewriting step on a VoxelScene -> the result in the model's form"""
    t = s["tool"]
    if t == "edit":
        return sc.edit(s["lo"], np.asarray(s["ids"], np.uint8))
    if t == "fill":
        return sc.fill(s["lo"], s["size"], s["id"])
    if t == "brush":
        return sc.brush(s["shape"], s["mode"], s["p"], s["id"], s["match"])
    if t == "stamp":
        return sc.stamp(s["dst"], sc if s["src"] == "self" else second, s["src_lo"], s["size"], s["orient"], s["skip_empty"])
    if t == "flood":
        return sc.flood(s["seed"], s["id"], s["match"], s["conn"], s["bounds"])
    if t == "morph":
        return sc.morph(s["op"], s["r"], s["conn"], s["id"], s["bounds"], s["border"])
    if t == "filter":
        return sc.filter_components(s["id"], s["match"], s["conn"], s["bounds"], **s["kw"])
    assert t == "voxelize", t
    return sc.voxelize(s["vertices"], s["triangles"], s["id"], s["mode"], s["fill"], s["bounds"], s["match"])


def ask(sc, s):
    """one reading step on a VoxelScene, for the kinds read_expected answers (components: (records, result) alone)"""
    t = s["tool"]
    if t == "read":
        return sc.read(s["lo"], s["size"])
    if t == "voxels":
        return sc.voxels(s["lo"], s["size"])
    if t == "count":
        return sc.count(s["lo"], s["size"])
    if t == "face_count":
        return sc.face_count(s["lo"], s["size"], s["runs"], s["closed"])
    if t == "faces":
        return sc.faces(s["lo"], s["size"], s["runs"], s["closed"])
    if t == "components":
        return sc.components(s["match"], s["conn"], s["bounds"])
    if t == "region":
        return sc.region(s["seed"], s["match"], s["conn"], s["bounds"])
    if t == "morph_measure":
        return sc.morph(s["op"], s["r"], s["conn"], s["id"], s["bounds"], s["border"], measure=True)
    assert t == "filter_measure", t
    return sc.filter_components(s["id"], s["match"], s["conn"], s["bounds"], measure=True, **s["kw"])


def same_answer(s, got, exp):
    t = s["tool"]
    if t in ("read", "voxels", "face_count"):
        return got.shape == exp.shape and bool((got == exp).all())
    if t == "faces":
        return got[0].shape == exp[0].shape and bool((got[0] == exp[0]).all()) and bool((got[1] == exp[1]).all())
    if t == "components":
        import components_common as cc
        rec = CR.records_array(exp[0], cc.DTYPE)
        return got[1] == exp[1] and all(bool((got[0][f] == rec[f]).all()) for f in ("root", "id", "voxels", "lo", "size", "faces"))
    return got == exp
