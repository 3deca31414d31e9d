"""Temporal reprojection, the definition restated in numpy: every fp32 step of csrc/vrt_reproject.h as one float32 array operation
(numpy rounds each to fp32: no contraction, IEEE division and square root), every integer step in uint64 (no sum of the
definition leaves 32 bits, so the width does not matter).  Shares no code with the header; tests/test_reproject_cpu.py compares
the two bit for bit, tests/test_gpu_reproject.py the kernel against this.

A history is (color16 uint16 [H, W, 4], surface uint32 [H, W, 4]); a push anything with cam_pos / cam_dir / cam_right / cam_up /
camera_jitter (ctypes Push blocks of the package or the oracle)."""
import numpy as np

F = np.float32
CLASSES = ("miss", "full", "partial", "disoccluded", "outside", "behind")


def _v3(a):
    return np.array([a[0], a[1], a[2]], F)


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def default_tol_rel(cur, W):
    r = _v3(cur.cam_right)
    return (F(4.0) * np.sqrt(_dot3(r, r))) / F(W)


def consts(W, H, prev):
    """R0, R1, R2, det of the previous camera (None: degenerate)."""
    with np.errstate(all="ignore"):
        fW, fH = F(W), F(H)
        cd = _v3(prev.cam_dir)
        l = np.sqrt(_dot3(cd, cd))
        cd = np.zeros(3, F) if l == 0 else (cd / l).astype(F)
        U = _v3(prev.cam_right)
        V = ((_v3(prev.cam_up) * fH) / fW).astype(F)
        jx = (F(prev.camera_jitter[0]) / fW) * F(-2.0)
        jy = (F(prev.camera_jitter[1]) / fH) * F(2.0)
        Cv = np.array([cd[0] + jx, cd[1] + jy, cd[2]], F)
        R0, R1, R2 = _cross(V, Cv), _cross(Cv, U), _cross(U, V)
        det = _dot3(U, R0)
    if not np.isfinite(det) or det == 0:
        return None
    return R0, R1, R2, det


def reproject(W, H, cur, prev, color8, position, normal8, hist=None, max_history=32, tol_abs=0.5, tol_rel=None):
    """One frame.  color8 uint8 [H, W, 4], position float32 [H, W, 4], normal8 int8 [H, W, 4]; hist: the previous frame's
    (color16, surface) or None.  Returns a dict: color16, surface, resolved8 uint8 [H, W, 4], motion float32 [H, W, 2], and cls,
    the class of every pixel (index into CLASSES)."""
    assert 1 <= max_history <= 255
    k = consts(W, H, prev)
    assert k is not None, "degenerate basis"
    R0, R1, R2, det = k
    tol_abs = F(tol_abs)
    tol_rel = default_tol_rel(cur, W) if tol_rel is None else F(tol_rel)
    c = np.ascontiguousarray(color8).reshape(H, W, 4).astype(np.uint64)
    pos_bits = np.ascontiguousarray(position, dtype=F).reshape(H, W, 4).view(np.uint32)
    P = pos_bits.view(F)[..., :3]
    N = np.ascontiguousarray(normal8).reshape(H, W, 4).view(np.uint8).astype(np.uint32)
    N = N[..., 0] | (N[..., 1] << 8) | (N[..., 2] << 16) | (N[..., 3] << 24)
    nbits = N & np.uint32(0xFFFFFF)
    miss = N == 0
    py, px = np.mgrid[0:H, 0:W]
    with np.errstate(all="ignore"):
        d = P - _v3(prev.cam_pos)
        a, b, l = _dot3(d, R0), _dot3(d, R1), _dot3(d, R2)
        front = np.isfinite(l) & (l != 0) & ((l > 0) == bool(det > 0)) & ~miss
        sx, sy = a / l, b / l
        qx = ((sx + F(1.0)) * F(0.5)) * F(W) - F(0.5)
        qy = ((sy + F(1.0)) * F(0.5)) * F(H) - F(0.5)
        motion = np.zeros((H, W, 2), F)
        motion[..., 0] = np.where(front, qx - px.astype(F), F(0))
        motion[..., 1] = np.where(front, qy - py.astype(F), F(0))
        taps = front & np.isfinite(qx) & np.isfinite(qy)
        if hist is None:
            taps = np.zeros_like(taps)
        x0f, y0f = np.floor(qx), np.floor(qy)
        wx = np.where(taps, np.floor((qx - x0f) * F(256.0) + F(0.5)), 0).astype(np.int64)
        wy = np.where(taps, np.floor((qy - y0f) * F(256.0) + F(0.5)), 0).astype(np.int64)
        x0 = np.where(taps, np.clip(x0f, F(-2.0), F(W)), 0).astype(np.int64)
        y0 = np.where(taps, np.clip(y0f, F(-2.0), F(H)), 0).astype(np.int64)
        dc = P - _v3(cur.cam_pos)
        tol = tol_abs + tol_rel * np.sqrt(_dot3(dc, dc))
        tol2 = tol * tol
        ws = np.zeros((H, W), np.uint64)
        acc = np.zeros((H, W, 4), np.uint64)
        cmin = np.full((H, W), 255, np.uint64)
        nonzero = np.zeros((H, W), np.int64)
        nvalid = np.zeros((H, W), np.int64)
        inside_any = np.zeros((H, W), bool)
        if hist is not None:
            h16 = np.ascontiguousarray(hist[0]).reshape(H, W, 4).astype(np.uint64)
            hs = np.ascontiguousarray(hist[1]).reshape(H, W, 4).view(np.uint32)
            hpos = hs.view(F)[..., :3]
            for t in range(4):
                tx, ty = x0 + (t & 1), y0 + (t >> 1)
                w = (wx if t & 1 else 256 - wx) * (wy if t >> 1 else 256 - wy)
                live = taps & (w != 0)
                inside = live & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
                s = hs[tyc, txc]
                e = hpos[tyc, txc] - P
                ok = inside & ((s[..., 3] & np.uint32(0xFFFFFF)) == nbits) & (_dot3(e, e) <= tol2)
                wv = np.where(ok, w, 0).astype(np.uint64)
                ws += wv
                acc += wv[..., None] * h16[tyc, txc]
                cmin = np.where(ok, np.minimum(cmin, (s[..., 3] >> 24).astype(np.uint64)), cmin)
                nonzero += live; nvalid += ok; inside_any |= inside
    has = ws != 0
    wsd = np.where(has, ws, 1)
    h = (acc + (ws // 2)[..., None]) // wsd[..., None]
    n = np.where(has, np.minimum(cmin + 1, np.uint64(max_history)), 1).astype(np.uint64)
    blended = (h * (n - 1)[..., None] + c * 256 + (n // 2)[..., None]) // n[..., None]
    color16 = np.where(has[..., None], blended, c * 256)
    surface = np.zeros((H, W, 4), np.uint32)
    surface[..., :3] = np.where(miss[..., None], np.uint32(0), pos_bits[..., :3])
    surface[..., 3] = np.where(miss, np.uint32(1 << 24), nbits | (n.astype(np.uint32) << 24))
    resolved = np.minimum((color16 + 128) >> 8, 255).astype(np.uint8)
    cls = np.full((H, W), 3, np.uint8)                                  # disoccluded: a hit without a valid tap
    cls[~miss & ~front] = 5
    cls[taps & ~inside_any] = 4
    cls[front & ~taps & (hist is not None)] = 4                         # projected to infinity
    cls[has & (nvalid < nonzero)] = 2
    cls[has & (nvalid == nonzero)] = 1
    cls[miss] = 0
    return {"color16": color16.astype(np.uint16), "surface": surface, "resolved8": resolved, "motion": motion, "cls": cls}


def shares(cls):
    return {name: float((cls == k).mean()) for k, name in enumerate(CLASSES)}


def same(a, b, names=("color16", "surface", "resolved8", "motion")):
    """Names of the planes that differ, motion by bit pattern."""
    bad = []
    for k in names:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, (k, x.shape, y.shape, x.dtype, y.dtype)
        if k == "motion":
            x, y = x.view(np.uint32), y.view(np.uint32)
        if not (x == y).all():
            bad.append((k, int((x != y).any(axis=-1).sum())))
    return bad
