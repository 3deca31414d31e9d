"""What the CPU and GPU tests of the connected components share: the small volumes built to break a tiled union-find (blobs inside
one tile, a plus through every face of a tile, diagonal contact on and off a tile edge, a U that joins in the neighbour tile, a
serpentine, a ring around the corner of eight tiles, a root reached last, touching ids, cavities, bounds off the tile grid, a
checkerboard, random volumes around the percolation threshold), the queries each is asked, and the reference's answers, computed
once and shared.  Volumes are uint8 arrays indexed [z, y, x]."""
import itertools

import numpy as np

import components_reference as R
import flood_common as fc

DTYPE = np.dtype([("root", np.int32, 3), ("id", np.uint32), ("voxels", np.uint64), ("lo", np.int32, 3), ("size", np.uint32, 3),
                  ("faces", np.uint32), ("reserved", np.uint32)])

BOTH_CONN = (R.FACES, R.CORNERS)
ALL = list(itertools.product((R.SOLID, R.SAME, R.EMPTY), BOTH_CONN, (None,)))
SOLID_ONLY = [(R.SOLID, 6, None), (R.SOLID, 26, None)]


def two_blobs():
    vol = np.zeros((24, 24, 24), np.uint8)
    vol[9:11, 9:11, 9:11] = 3
    vol[13:15, 12:14, 13:15] = 4                                  # both inside the middle tile, apart under 26 too
    return vol


def u_volume():
    """16 x 8 x 8: two arms along x that are separate inside tile 0 and joined by a bar at x = 9, inside tile 1"""
    vol = np.zeros((8, 8, 16), np.uint8)
    vol[3, 2, 2:10] = 6; vol[3, 5, 2:10] = 6; vol[3, 2:6, 9] = 6
    return vol


def ring_volume():
    """16^3: two stacked square rings around the corner (8, 8, 8) that eight tiles share: every tile holds a piece, the unions form cycles"""
    vol = np.zeros((16, 16, 16), np.uint8)
    vol[7:9, 6:10, 6:10] = 5
    vol[7:9, 7:9, 7:9] = 0
    return vol


def late_root_volume():
    """24^3: a body filling tile (1, 1, 1) and one voxel at (7, 7, 7), the last voxel of tile (0, 0, 0): under 26 it is the root of
    the whole and touches it at a corner only; and a path whose root at (1, 1, 1) is joined to its tile's other piece only through
    tiles further on"""
    vol = np.zeros((24, 24, 24), np.uint8)
    vol[8:16, 8:16, 8:16] = 2
    vol[7, 7, 7] = 2
    vol[1, 1, 1:20] = 7; vol[1:20, 1, 19] = 7; vol[19, 1:20, 19] = 7; vol[19, 19, 3:20] = 7; vol[3:20, 19, 3] = 7; vol[3, 3:20, 3] = 7     # a spiral back into tile (0, 0, 0)
    return vol


def touching_ids():
    vol = np.zeros((16, 16, 16), np.uint8)
    vol[4:12, 4:12, 3:8] = 1
    vol[4:12, 4:12, 8:13] = 2                                     # the contact is a tile plane
    vol[2, 2, 2] = 2
    return vol


def cavities():
    """40 x 24 x 32: flood's leaking hollow box, and a closed one beside it"""
    vol, _, _ = fc.cavity_volume()
    vol[24:30, 6:16, 30:38] = 9
    vol[25:29, 7:15, 31:37] = 0
    return vol


def checkerboard():
    z, y, x = np.indices((16, 16, 16))
    return (((x + y + z) & 1) * 3).astype(np.uint8)


def random_volume(p, seed):
    return fc.random_volume((40, 40, 40), p, seed)


OFF_GRID = [((3, 5, 1), (17, 9, 21)), ((-4, -2, -3), (20, 30, 15)), ((30, 30, 30), (100, 100, 100))]

# name -> (volume maker, queries)
CASES = {
    "two_blobs": (two_blobs, ALL),
    "plus": (lambda: fc.plus_volume()[0], ALL),
    "edge8": (lambda: fc.diagonal_volume("edge", 8)[0], SOLID_ONLY), "edge12": (lambda: fc.diagonal_volume("edge", 12)[0], SOLID_ONLY),
    "corner8": (lambda: fc.diagonal_volume("corner", 8)[0], SOLID_ONLY), "corner12": (lambda: fc.diagonal_volume("corner", 12)[0], SOLID_ONLY),
    "u": (u_volume, SOLID_ONLY + [(R.EMPTY, 6, None)]),
    "serpentine": (lambda: fc.serpentine_volume()[0], ALL),
    "ring": (ring_volume, ALL),
    "late_root": (late_root_volume, ALL),
    "touching_ids": (touching_ids, ALL),
    "cavities": (cavities, [(R.EMPTY, 6, None), (R.EMPTY, 26, None), (R.SOLID, 6, None)]),
    "off_grid": (lambda: random_volume(0.31, 5), [(m, c, b) for (m, c), b in itertools.product(((R.SOLID, 6), (R.SAME, 26), (R.EMPTY, 6)), OFF_GRID)]),
    "checkerboard": (checkerboard, SOLID_ONLY + [(R.EMPTY, 6, None)]),
}
for _p, _seed in itertools.product((0.25, 0.31, 0.4), (1, 2)):
    CASES[f"random_{_p}_{_seed}"] = ((lambda p=_p, s=_seed: random_volume(p, s)), ALL)

_volumes, _answers = {}, {}


def volume(name):
    if name not in _volumes:
        _volumes[name] = CASES[name][0]()
        _volumes[name].setflags(write=False)
    return _volumes[name]


def answer(name, match, conn, bounds):
    """the reference's (records as a structured array, result, labels, (clo, csize)) for a query of a case: computed once"""
    k = (name, match, conn, bounds)
    if k not in _answers:
        records, result, labels, cl = R.components(volume(name), match, conn, bounds)
        if labels is not None:
            labels.setflags(write=False)
        _answers[k] = (R.records_array(records, DTYPE), result, labels, cl)
    return _answers[k]


def assert_same(got_records, got_result, got_labels, exp, what):
    exp_records, exp_result, exp_labels, _ = exp
    assert got_result == exp_result, (what, got_result, exp_result)
    assert got_records.dtype == exp_records.dtype and got_records.tobytes() == exp_records.tobytes(), (what, got_records[:4], exp_records[:4])
    if exp_labels is None:
        assert got_labels is None, what
    else:
        assert got_labels.shape == exp_labels.shape and (got_labels == exp_labels).all(), what
