"""The definition vrt_scene_morph is held to (csrc/vrt_morph.h), twice over, in numpy and Python integers: the CLOSED FORM (a cell
is in dil_r(X) iff some cell of X lies within distance r of it: brute force over the ball's offsets) and r UNIT STEPS of the
connectivity's neighbourhood.  No masks, no tiles, no row words.  Volumes are uint8 arrays indexed [z, y, x]; sets are bool arrays
over a WINDOW of the infinite grid, everything outside the window being one value (`fill`)."""
import numpy as np

DILATE, ERODE, OPEN, CLOSE, HOLLOW = 0, 1, 2, 3, 4
OPS = {"dilate": DILATE, "erode": ERODE, "open": OPEN, "close": CLOSE, "hollow": HOLLOW}
FACES, CORNERS = 6, 26
BORDER_SOLID, MEASURE = 1, 2
MAX_RADIUS, MAX_SIDE, MAX_SIZE = 8, 512, 1 << 30
ZERO = {"added": 0, "removed": 0, "changed": 0, "lo": (0, 0, 0), "size": (0, 0, 0)}


def adds(op):
    return op in (DILATE, CLOSE)


def halo(op, r):
    return 2 * r if op in (OPEN, CLOSE) else r


def args_ok(op, conn, r, flags, vid, size):
    return (op in (DILATE, ERODE, OPEN, CLOSE, HOLLOW) and conn in (FACES, CORNERS) and 1 <= int(r) <= MAX_RADIUS and (flags & ~(BORDER_SOLID | MEASURE)) == 0
            and (not adds(op) or 1 <= int(vid) <= 255) and all(1 <= int(s) <= MAX_SIZE for s in size))


def clip(lo, size, dims):
    """[lo, lo + size) cut to the volume -> (lo, size), or None when nothing is left"""
    l = [max(0, int(lo[a])) for a in range(3)]
    h = [min(int(dims[a]), int(lo[a]) + int(size[a])) for a in range(3)]
    if any(h[a] <= l[a] for a in range(3)):
        return None
    return l, [h[a] - l[a] for a in range(3)]


def dist(conn, d):
    return sum(abs(int(t)) for t in d) if conn == FACES else max(abs(int(t)) for t in d)


def ball(conn, r):
    """the offsets (dx, dy, dz) within distance r: L1 under 6, L-infinity under 26"""
    rr = range(-r, r + 1)
    return [(dx, dy, dz) for dz in rr for dy in rr for dx in rr if dist(conn, (dx, dy, dz)) <= r]


def dil_closed(X, conn, r, fill):
    """dil_r of the window X, whose outside is `fill` everywhere: the OR over the ball's offsets"""
    D, H, W = X.shape
    P = np.pad(X, r, constant_values=bool(fill))
    out = np.zeros_like(X)
    for dx, dy, dz in ball(conn, r):
        out |= P[r + dz:r + dz + D, r + dy:r + dy + H, r + dx:r + dx + W]
    return out


def dil_steps(X, conn, r, fill):
    """r applications of the unit step"""
    for _ in range(r):
        X = dil_closed(X, conn, 1, fill)
    return X


def dil(X, conn, r, fill, how):
    return (dil_closed if how == "closed" else dil_steps)(X, conn, r, fill)


def ero(X, conn, r, fill, how):
    """every cell whose whole ball lies in X: the complement's dilation, complemented"""
    return ~dil(~X, conn, r, not fill, how)


def result_set(vol, op, conn, r, border_solid=False, how="steps"):
    """R over the volume, bool [z, y, x].  The window is the volume and 2r + 1 cells around it, so whatever is not uniform stays
    inside it through both phases: outside the window every intermediate set is the border's value."""
    b, p = bool(border_solid), 2 * r + 1
    S = np.pad(vol != 0, p, constant_values=b)
    if op == DILATE:
        R = dil(S, conn, r, b, how)
    elif op == ERODE:
        R = ero(S, conn, r, b, how)
    elif op == OPEN:
        R = dil(ero(S, conn, r, b, how), conn, r, b, how)
    elif op == CLOSE:
        R = ero(dil(S, conn, r, b, how), conn, r, b, how)
    else:
        R = S & ~ero(S, conn, r, b, how)
    return R[p:-p, p:-p, p:-p]


def tight(mask):
    n = int(mask.sum())
    if n == 0:
        return 0, (0, 0, 0), (0, 0, 0)
    zs, ys, xs = np.nonzero(mask)
    lo = (int(xs.min()), int(ys.min()), int(zs.min()))
    return n, lo, (int(xs.max()) - lo[0] + 1, int(ys.max()) - lo[1] + 1, int(zs.max()) - lo[2] + 1)


def morph(vol, op, r, conn=FACES, vid=0, bounds=None, border_solid=False, measure=False, how="steps"):
    """-> (the volume after, the result as VoxelScene.morph returns it); vol itself is left alone"""
    op = OPS[op] if isinstance(op, str) else op
    D, H, W = vol.shape
    lo, size = ((0, 0, 0), (W, H, D)) if bounds is None else bounds
    assert args_ok(op, conn, r, 0, vid, size)
    box = clip(lo, size, (W, H, D))
    if box is None:
        return vol.copy(), dict(ZERO)
    (x0, y0, z0), (nx, ny, nz) = box
    assert max(nx, ny, nz) <= MAX_SIDE
    R = result_set(vol, op, conn, r, border_solid, how)
    inb = np.zeros(vol.shape, bool)
    inb[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = True
    add, rem = inb & R & (vol == 0), inb & ~R & (vol != 0)
    out = vol.copy()
    res = dict(ZERO, added=int(add.sum()), removed=int(rem.sum()))
    if not measure:
        out[add] = vid
        out[rem] = 0
        res["changed"], res["lo"], res["size"] = tight(out != vol)
    return out, res
