"""What the tests of vrt_scene_list_faces share: the volumes, the table of boxes (the GPU tests run it on the device, the CPU tests
on the host build of csrc/vrt_faces.h), and the reference's records by case, computed once."""
import numpy as np

import faces_reference as R

KINDS = ("dense", "reserved", "unreserved")


def _random(dims, seed, density=0.5, ids=3):
    W, H, D = dims
    rng = np.random.default_rng(seed)
    return ((rng.random((D, H, W)) < density) * rng.integers(1, ids + 1, (D, H, W))).astype(np.uint8)


def _bars(dims):
    """a bar of id 9 along x over box-relative x 3 .. 132 and one of id 11 along y over box-relative y 3 .. 132 (the box starts at 1, 1, 1)"""
    W, H, D = dims
    vol = np.zeros((D, H, W), np.uint8)
    vol[3, 3, 4:134] = 9
    vol[3, 4:134, 137] = 11
    return vol


def _alternating(dims):
    W, H, D = dims
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    return np.where(z == 3, np.where((x + y) % 2 == 0, 1, 255), 0).astype(np.uint8)


def _checker(dims):
    W, H, D = dims
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    return (((x + y + z) % 2) * 9).astype(np.uint8)


def _corner_brick(dims):
    W, H, D = dims
    vol = np.zeros((D, H, W), np.uint8)
    vol[0:8, 0:8, 0:8] = _random((8, 8, 8), 4)
    return vol


# name -> (dims (W, H, D), each a multiple of 8 so that the volume is a brick scene too, builder)
VOLUMES = {
    "long-x": ((264, 8, 8), lambda d: _random(d, 1)),
    "long-y": ((8, 264, 8), lambda d: _random(d, 2)),
    "bars": ((144, 144, 8), _bars),
    "alternating": ((72, 8, 8), _alternating),
    "random": ((72, 48, 56), lambda d: _random(d, 3)),
    "solid": ((24, 24, 24), lambda d: np.full((d[2], d[1], d[0]), 7, np.uint8)),
    "corner-brick": ((32, 32, 32), _corner_brick),
    "checker": ((64, 8, 8), _checker),
}
RANDOM_BOX = ((1, 3, 1), (70, 45, 52))                 # 70 x 45 x 52 inside 72 x 48 x 56: no face of the box on the brick grid

# (case, volume, lo, size): every box at an odd lo unless it is the whole volume
CASES = [("one voxel", "long-x", (5, 3, 1), (1, 1, 1))]
CASES += [(f"x {n}", "long-x", (3, 1, 1), (n, 5, 3)) for n in (63, 64, 65, 256)]
CASES += [(f"y {n}", "long-y", (1, 3, 1), (5, n, 3)) for n in (63, 64, 65, 256)]
CASES += [("bars", "bars", (1, 1, 1), (140, 140, 5)),
          ("alternating ids", "alternating", (0, 0, 0), (72, 8, 8)),
          ("random", "random") + RANDOM_BOX,
          ("every volume face", "random", (0, 0, 0), (72, 48, 56)),
          ("inside solid material", "solid", (5, 5, 5), (9, 10, 11)),
          ("over empty bricks", "corner-brick", (9, 9, 9), (20, 20, 20)),
          ("checkerboard", "checker", (0, 0, 0), (64, 8, 8))]
FLAGS = [(False, False), (True, False), (False, True), (True, True)]        # (runs, closed)

_volumes, _expected = {}, {}


def volume(name):
    if name not in _volumes:
        dims, make = VOLUMES[name]
        v = np.ascontiguousarray(make(dims), np.uint8)
        assert v.shape == dims[::-1]
        v.setflags(write=False)
        _volumes[name] = v
    return _volumes[name]


def expected(vol_name, lo, size, runs, closed):
    """the reference's (records, counts) of a box of a named volume, computed once"""
    key = (vol_name, tuple(lo), tuple(size), bool(runs), bool(closed))
    if key not in _expected:
        rec, counts = R.faces(volume(vol_name), lo, size, runs, closed)
        rec.setflags(write=False)
        _expected[key] = (rec, counts)
    return _expected[key]


def eight_parts(lo, size):
    """the box cut in two along every axis, unevenly -> eight (lo, size)"""
    cuts = [(0, size[a] // 2 + 1, size[a]) for a in range(3)]
    return [(tuple(lo[a] + cuts[a][i[a]] for a in range(3)), tuple(cuts[a][i[a] + 1] - cuts[a][i[a]] for a in range(3)))
            for i in np.ndindex(2, 2, 2)]


def make_scene(vrt, engine, vol, pal, kind):
    if kind == "dense":
        return vrt.VoxelScene.from_dense(engine, vol, pal)
    grid, pool = vrt.synthetic.bricks_from_dense(vol)
    sc = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
    if kind == "reserved":
        sc.reserve_bricks(pool.shape[0] + 16)
    return sc
