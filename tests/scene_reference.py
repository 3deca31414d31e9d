"""What a fresh scene build must contain, in plain numpy: the definitions of the device structures vrt_scene_from_dense and
vrt_scene_from_bricks build (include/vrt.h VRT_STATE_*), written from the volume alone -- no three-pass min-max transform, nothing
taken from csrc/ but the caps, which are read from the headers so that a changed cap moves the reference with it.

vol[z, y, x] is a uint8 volume, 0 = empty; outside the volume counts as solid.  An octant o has the signs
sx = +1 if o & 1 else -1, sy from bit 1, sz from bit 2.

The second half holds the comparers the GPU tests (tests/test_gpu_scene_build.py) judge a downloaded structure with; each returns
None or a message that names the field / word and the coordinates of the first difference (tests/test_scene_reference_cpu.py
checks that they see single-byte and single-bit slips)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxel-raytracing_amd", "csrc")


def _define(header, name):
    return int(re.search(r"#define %s (\d+)" % name, open(os.path.join(CSRC, header)).read()).group(1))


DF_CAP = _define("vrt_device_common.h", "VRT_DF_CAP")
FINE_CAP = _define("vrt_scene_build.hip", "VRT_FINE_CAP")
BRICK_CAP = _define("vrt_brick_edit.h", "VRT_BRICK_EDIT_CAP")
PTR_MASK = np.uint64(0xFFFFFF)
PTR_BORDER = 0xFFFFFF


def signs(o):
    return (1 if o & 1 else -1), (1 if o & 2 else -1), (1 if o & 4 else -1)


def _flip_to_positive(a, o):
    """the array seen from octant o's corner: afterwards the octant extends towards +x, +y, +z"""
    sx, sy, sz = signs(o)
    axes = [ax for ax, s in ((2, sx), (1, sy), (0, sz)) if s < 0]
    return np.flip(a, axes) if axes else a


def clearance(vol, o, cap):
    """c[z, y, x]: the side of the largest all-empty axis-aligned cube that has one corner voxel at p and extends towards
    (sx, sy, sz), lies wholly inside the volume, capped at `cap`; 0 at a solid voxel.  By erosion: E_1 = empty, E_k(p) = AND of
    E_{k-1} over the eight offsets {0, 1}^3 . s (taken one axis after the other), c = #{k <= cap : E_k(p)}.  In the flipped
    array E_k has one cell less per axis than E_{k-1}: a cube of side k at p fits the volume iff p <= dim - k."""
    e = _flip_to_positive(np.asarray(vol) == 0, o)
    c = np.zeros(e.shape, np.int32)
    for k in range(1, int(cap) + 1):
        if e.size == 0 or not e.any():
            break
        c[:e.shape[0], :e.shape[1], :e.shape[2]] += e
        e = e[:-1] & e[1:]
        e = e[:, :-1] & e[:, 1:]
        e = e[:, :, :-1] & e[:, :, 1:]
    return np.ascontiguousarray(_flip_to_positive(c, o)).astype(np.uint8 if cap < 256 else np.int32)


def open_cells(vol, o):
    """open[z, y, x]: no solid voxel in the whole box from p to the volume's corner in the octant (p itself included) -- the
    definition of tests/test_skip_soundness_cpu.py, which shows that a ray standing on such a cell hits nothing."""
    e = _flip_to_positive(np.asarray(vol) == 0, o)
    for axis in range(3):                                         # AND over everything at or beyond p along the axis
        e = np.flip(np.logical_and.accumulate(np.flip(e, axis), axis), axis)
    return np.ascontiguousarray(_flip_to_positive(e, o))


def df_field_bytes(W, H, D):
    return ((W + 2) * (H + 2) * (D + 2) + 255) & ~255


def dense_fields(vol, open):
    """the interiors of the eight fields, [o, z, y, x]"""
    out = np.empty((8,) + vol.shape, np.uint8)
    for o in range(8):
        c = clearance(vol, o, DF_CAP)
        if open:
            c[open_cells(vol, o)] = 0
        out[o] = c
    return out


def dense_df_bytes(vol, open, fields=None):
    """VRT_STATE_DF of a scene whose layout has the ninth field (every volume whose nine fields fit 32-bit offsets): eight fields of
    df_field_bytes each, x-fastest with a one-voxel border of zeros, the interior clearance(., o, VRT_DF_CAP) -- 0 where `open` is
    set and the cell is open --; the voxel ids in the same layout as field 8; one byte 0xFF at 9 * ndf; 255 zero bytes.  Every
    rounding tail is zero."""
    D, H, W = vol.shape
    ndf = df_field_bytes(W, H, D)
    out = np.zeros(9 * ndf + 256, np.uint8)
    f = dense_fields(vol, open) if fields is None else fields
    n = (W + 2) * (H + 2) * (D + 2)
    for o in range(9):
        out[o * ndf:o * ndf + n].reshape(D + 2, H + 2, W + 2)[1:-1, 1:-1, 1:-1] = f[o] if o < 8 else vol
    out[9 * ndf] = 0xFF
    return out


_BIT = (np.arange(4)[None, None, :] | (np.arange(4)[None, :, None] << 2) | (np.arange(4)[:, None, None] << 4)).astype(np.uint64)


def _level_up(nz):
    """nz[z, y, x] bool -> one uint64 per 4^3 block [ceil(z/4), ceil(y/4), ceil(x/4)], bit x | y << 2 | z << 4 of the block set where nz is"""
    d, h, w = nz.shape
    p = np.zeros(((d + 3) // 4 * 4, (h + 3) // 4 * 4, (w + 3) // 4 * 4), bool)
    p[:d, :h, :w] = nz
    b = p.reshape(p.shape[0] // 4, 4, p.shape[1] // 4, 4, p.shape[2] // 4, 4).transpose(0, 2, 4, 1, 3, 5)
    return (b * (np.uint64(1) << _BIT)).sum(axis=(3, 4, 5), dtype=np.uint64)


def pyramid(vol):
    """(OCC1, OCC2, OCC3) as they lie in memory: OCC1 one word per 4^3 cell of voxels, OCC2 / OCC3 the same rule over the non-zero
    words of the level below, each of the two padded with a zero word to an even count of words."""
    l1 = _level_up(np.asarray(vol) != 0)
    l2 = _level_up(l1 != 0)
    l3 = _level_up(l2 != 0)
    pad = lambda a: np.concatenate([a.reshape(-1), np.zeros(a.size & 1, np.uint64)])
    return l1.reshape(-1), pad(l2), pad(l3)


def cells(vol):
    """VRT_STATE_CELLS of a dense scene, sorted: x | y << 10 | z << 20 of the 4^3 cells that hold a voxel"""
    z, y, x = np.nonzero(_level_up(np.asarray(vol) != 0))
    return np.sort((x | (y << 10) | (z << 20)).astype(np.uint32))


def brick_occupancy(vol):
    D, H, W = vol.shape
    return vol.reshape(D // 8, 8, H // 8, 8, W // 8, 8).any(axis=(1, 3, 5))


def brick_cells(vol):
    """VRT_STATE_CELLS of a brick scene, sorted: the occupied bricks"""
    z, y, x = np.nonzero(brick_occupancy(vol))
    return np.sort((x | (y << 10) | (z << 20)).astype(np.uint32))


def brick_entries(grid, open):
    """VRT_STATE_BENTRY: one word per brick of the padded grid [nbz + 2, nby + 2, nbx + 2], flattened.  grid[bz, by, bx]: 0 for an
    empty brick, else 1 + its pool slot.
      bits 0..23   the pointer: 0 empty, 0xFFFFFF border, else the grid's value
      bit 24 + o   open: open_cells of the brick occupancy; never for an occupied or a border brick, nor when `open` is off
      bits 32 + 4 o .. 35 + 4 o   min(15, clearance(occupancy, o, VRT_BRICK_EDIT_CAP)); 0 for an occupied brick and the border"""
    grid = np.asarray(grid)
    occ = (grid != 0).astype(np.uint8)
    e = grid.astype(np.uint64) & PTR_MASK
    for o in range(8):
        e |= np.minimum(clearance(occ, o, BRICK_CAP), 15).astype(np.uint64) << np.uint64(32 + 4 * o)
        if open:
            e |= open_cells(occ, o).astype(np.uint64) << np.uint64(24 + o)
    out = np.full(tuple(n + 2 for n in grid.shape), np.uint64(PTR_BORDER), np.uint64)
    out[1:-1, 1:-1, 1:-1] = e
    return out.reshape(-1)


def brick_fine(vol, o):
    """f[z, y, x], meaningful for the voxels of occupied bricks: min(VRT_FINE_CAP, clearance(vol, o, VRT_FINE_CAP), window_x,
    window_y, window_z).

    The device looks from a brick through its 26 neighbours only: a 24^3 window in which the brick's voxel with local coordinate
    l in 0..7 sits at 8 + l, and everything beyond the window counts as solid, as everything outside the volume does (the comment
    above brick_fine_body in csrc/vrt_scene_build.hip: "beyond them ... counts as solid, so values reach 9..16").  Inside the
    window the voxels are the volume's, so a cube of side k at p is empty there iff it is empty in the volume AND fits the window,
    and it fits the window iff k <= the number of window cells from p to the window's edge along each axis of the octant:
    24 - (8 + l) = 16 - l for a positive step, (8 + l) + 1 = l + 9 for a negative one.  The largest such k is the minimum of the
    volume's clearance and the three window distances; all of them are <= 16 = VRT_FINE_CAP.  (In an occupied brick the value
    stays below 16: a window of 16 along all three axes means a cube that starts in a corner of the brick and covers all of it.)"""
    D, H, W = vol.shape
    c = clearance(vol, o, FINE_CAP).astype(np.int32)
    win = []
    for n, s in zip((W, H, D), signs(o)):
        l = np.arange(n) & 7
        win.append(16 - l if s > 0 else l + 9)
    c = np.minimum(c, win[0][None, None, :])
    c = np.minimum(c, win[1][None, :, None])
    c = np.minimum(c, win[2][:, None, None])
    return np.minimum(c, FINE_CAP).astype(np.uint8)


def to_bricks(a):
    """[z, y, x] -> [bz, by, bx, 512] with x + 8 y + 64 z inside the brick"""
    D, H, W = a.shape
    return a.reshape(D // 8, 8, H // 8, 8, W // 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(D // 8, H // 8, W // 8, 512)


def brick_fine_by_brick(vol):
    """[bz, by, bx, o, 512]; a scene holds it at [slot, o, x + 8 y + 64 z] for the slot an occupied brick's entry points to"""
    return np.stack([to_bricks(brick_fine(vol, o)) for o in range(8)], axis=3)


class PointReference:
    """Clearance and open cells at single points of a volume too large for whole-field references.  Both are statements about
    `vol[box].any()`; for 10^5 boxes of up to half a volume of 832^3 that test is answered from a summed-area table of the solid
    voxels (count of the box > 0), which tests/test_scene_reference_cpu.py holds against the literal slice test."""

    def __init__(self, vol):
        self.vol = vol
        D, H, W = vol.shape
        s = np.zeros((D + 1, H + 1, W + 1), np.int32)
        s[1:, 1:, 1:] = vol != 0
        for a in range(3):
            np.cumsum(s, axis=a, out=s)
        self.sat = s

    def box_any(self, lo, hi):
        """vol[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]].any(); lo, hi = (x, y, z), inside the volume, lo < hi"""
        (x0, y0, z0), (x1, y1, z1), s = lo, hi, self.sat
        n = (int(s[z1, y1, x1]) - int(s[z0, y1, x1]) - int(s[z1, y0, x1]) - int(s[z1, y1, x0])
             + int(s[z0, y0, x1]) + int(s[z0, y1, x0]) + int(s[z1, y0, x0]) - int(s[z0, y0, x0]))
        return n > 0

    def _box(self, p, o, k):
        """the cube of side k (or, k = None, the box to the volume's corner) at p towards octant o, as (lo, hi)"""
        D, H, W = self.vol.shape
        lo, hi = [], []
        for c, n, s in zip(p, (W, H, D), signs(o)):
            if s > 0:
                lo.append(c); hi.append(n if k is None else c + k)
            else:
                lo.append(0 if k is None else c - k + 1); hi.append(c + 1)
        return lo, hi

    def clearance(self, p, o, cap):
        """p = (x, y, z).  The largest k <= cap whose cube is inside the volume and empty; emptiness is monotone in k, so a
        binary search finds it"""
        D, H, W = self.vol.shape
        fit = min(n - c if s > 0 else c + 1 for c, n, s in zip(p, (W, H, D), signs(o)))      # the walls: explicit
        good, bad = 0, min(cap, fit) + 1
        while bad - good > 1:
            k = (good + bad) // 2
            if self.box_any(*self._box(p, o, k)):
                bad = k
            else:
                good = k
        return good

    def open(self, p, o):
        return not self.box_any(*self._box(p, o, None))


# ---- comparers ------------------------------------------------------------------------------------------------------------------

def describe_df_offset(i, dims, fields=9):
    """where byte i of a VRT_STATE_DF allocation lies"""
    W, H, D = dims
    ndf, n = df_field_bytes(W, H, D), (W + 2) * (H + 2) * (D + 2)
    f, r = divmod(int(i), ndf)
    if f >= fields:
        return "the 0xFF byte behind field 8" if (f, r) == (9, 0) else f"tail byte {r} behind the 0xFF byte"
    if r >= n:
        return f"field {f} rounding tail byte {r - n}"
    x, y, z = r % (W + 2) - 1, r // (W + 2) % (H + 2) - 1, r // ((W + 2) * (H + 2)) - 1
    border = not (0 <= x < W and 0 <= y < H and 0 <= z < D)
    return f"field {f} x {x} y {y} z {z}" + (" (border)" if border else "")


def diff_df(got, expect, dims, what=""):
    if got.shape != expect.shape:
        return f"{what}: DF holds {got.size} bytes, expected {expect.size}"
    i = np.flatnonzero(got != expect)
    if i.size == 0:
        return None
    return f"{what}: DF differs in {i.size} places, first at {int(i[0])}, {describe_df_offset(i[0], dims)}: {int(got[i[0]])} != {int(expect[i[0]])}"


def level_dims(dims, level):
    """(nx, ny, nz) of pyramid level 1..3 of a W x H x D volume"""
    for _ in range(level):
        dims = tuple((n + 3) // 4 for n in dims)
    return dims


def diff_words(got, expect, name, n, what=""):
    """a pyramid level: words [z, y, x] flattened (n = (nx, ny, nz): its extent), perhaps with a padding word behind"""
    nx, ny, nz = n
    if got.shape != expect.shape:
        return f"{what}: {name} holds {got.size} words, expected {expect.size}"
    i = np.flatnonzero(got != expect)
    if i.size == 0:
        return None
    w = int(i[0])
    bits = int(got[w]) ^ int(expect[w])
    b = (bits & -bits).bit_length() - 1
    at = f"word x {w % nx} y {w // nx % ny} z {w // (nx * ny)}" if w < nx * ny * nz else "the padding word"
    return f"{what}: {name} differs in {i.size} words, first at {w}, {at}, bit {b} (x {b & 3} y {b >> 2 & 3} z {b >> 4}): {int(got[w]):#x} != {int(expect[w]):#x}"


def diff_cells(got, expect, what=""):
    got = np.sort(got)
    if got.shape != expect.shape or (got != expect).any():
        odd = np.setxor1d(got, expect)
        c = int(odd[0]) if odd.size else -1
        return f"{what}: CELLS holds {got.size} cells, expected {expect.size}; first odd one x {c & 1023} y {c >> 10 & 1023} z {c >> 20}"
    return None


def diff_entries(got, expect, nb, slots=None, what=""):
    """VRT_STATE_BENTRY against brick_entries().  nb = (nbx, nby, nbz).  slots None: the pointers must be the grid's own (a fresh
    build keeps them); a number: occupied, distinct and at most that many (a reserved scene may move a brick to another slot)."""
    if got.shape != expect.shape:
        return f"{what}: BENTRY holds {got.size} words, expected {expect.size}"
    pbx, pby = nb[0] + 2, nb[1] + 2
    at = lambda i: f"padded index {int(i)} (brick x {int(i) % pbx - 1} y {int(i) // pbx % pby - 1} z {int(i) // (pbx * pby) - 1})"
    ga, ea = got & ~PTR_MASK, expect & ~PTR_MASK
    i = np.flatnonzero(ga != ea)
    if i.size:
        bits = int(ga[i[0]]) ^ int(ea[i[0]])
        b = (bits & -bits).bit_length() - 1
        group = f"open bit of octant {b - 24}" if b < 32 else f"coarse clearance of octant {(b - 32) // 4}"
        return f"{what}: BENTRY differs in {i.size} words, first at {at(i[0])}, {group}: {int(got[i[0]]):#x} != {int(expect[i[0]]):#x}"
    gp, ep = (got & PTR_MASK).astype(np.int64), (expect & PTR_MASK).astype(np.int64)
    if slots is None:
        i = np.flatnonzero(gp != ep)
    else:
        kind = lambda p: np.where(p == 0, 0, np.where(p == PTR_BORDER, 2, 1))
        i = np.flatnonzero(kind(gp) != kind(ep))
        if i.size == 0:
            occ = np.flatnonzero(kind(gp) == 1)
            i = occ[gp[occ] > slots]
            if i.size == 0:
                _, first, count = np.unique(gp[occ], return_index=True, return_counts=True)
                i = np.sort(occ[first[count > 1]])
    if i.size:
        return f"{what}: BENTRY differs in {i.size} words, first at {at(i[0])}, pointer: {int(gp[i[0]]):#x} != {int(ep[i[0]]):#x}"
    return None


def diff_brick_bytes(entries, pool, fine, vol, nb, what=""):
    """the pool's ids and the per-voxel clearances of every occupied brick, through the pointer of its entry"""
    nbx, nby, nbz = nb
    ptr = (entries & PTR_MASK).astype(np.int64).reshape(nbz + 2, nby + 2, nbx + 2)[1:-1, 1:-1, 1:-1]
    ids, ref = to_bricks(vol), brick_fine_by_brick(vol)
    occ = brick_occupancy(vol)
    if ((ptr != 0) != occ).any():
        z, y, x = (int(v[0]) for v in np.nonzero((ptr != 0) != occ))
        return f"{what}: brick x {x} y {y} z {z} is {'occupied' if occ[z, y, x] else 'empty'} but its pointer is {int(ptr[z, y, x])}"
    if occ.any() and (int(ptr[occ].max()) > pool.shape[0] or fine.shape[0] != pool.shape[0]):
        return f"{what}: a pointer past the pool ({int(ptr[occ].max())} > {pool.shape[0]} slots, {fine.shape[0]} of clearances)"
    for z, y, x in zip(*np.nonzero(occ)):
        s = int(ptr[z, y, x]) - 1
        if (pool[s] != ids[z, y, x]).any():
            t = int(np.flatnonzero(pool[s] != ids[z, y, x])[0])
            return f"{what}: BPOOL slot {s} (brick x {x} y {y} z {z}) voxel x {t & 7} y {t >> 3 & 7} z {t >> 6}: {int(pool[s][t])} != {int(ids[z, y, x][t])}"
        if (fine[s] != ref[z, y, x]).any():
            o, t = (int(v[0]) for v in np.nonzero(fine[s] != ref[z, y, x]))
            n = int((fine[s] != ref[z, y, x]).sum())
            return (f"{what}: BFINE slot {s} (brick x {x} y {y} z {z}) differs in {n} bytes, first at octant {o} voxel x {t & 7} y {t >> 3 & 7} z {t >> 6}: "
                    f"{int(fine[s][o, t])} != {int(ref[z, y, x][o, t])}")
    return None
