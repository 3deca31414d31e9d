"""Temporal upsampling, the definition restated in numpy: every fp32 step of csrc/vrt_upsample.h as one float32 array operation
(numpy rounds each to fp32: no contraction, IEEE division and square root), every integer step in uint64 (no sum of the
definition leaves 32 bits, so the width does not matter).  Shares no code with the header; tests/test_upsample_cpu.py compares
the two bit for bit, tests/test_gpu_upsample.py the kernel against this.

The frame is w x h, the history (color16 uint16 [TH, TW, 4], surface uint32 [TH, TW, 4]) and every output TW x TH; a push is
anything with cam_pos / cam_dir / cam_right / cam_up (its camera_jitter is not read: both projections are unjittered)."""
import numpy as np

from reproject_reference import F, _cross, _dot3, _v3, default_tol_rel, same  # noqa: F401  (same: re-exported)

CLASSES = ("miss", "full", "partial", "disoccluded", "outside", "behind")
WEIGHTS = ("sampled", "carried")


def camera(w, h, push):
    """R0, R1, R2, det of push's camera without jitter, plane vector V = camUp * h / w (None: degenerate)."""
    with np.errstate(all="ignore"):
        fw, fh = F(w), F(h)
        cd = _v3(push.cam_dir)
        l = np.sqrt(_dot3(cd, cd))
        Cv = np.zeros(3, F) if l == 0 else (cd / l).astype(F)
        U = _v3(push.cam_right)
        V = ((_v3(push.cam_up) * fh) / fw).astype(F)
        R0, R1, R2 = _cross(V, Cv), _cross(Cv, U), _cross(U, V)
        det = _dot3(U, R0)
    if not np.isfinite(det) or det == 0:
        return None
    return R0, R1, R2, det


def source(w, h, TW, TH):
    """(ry, rx) index arrays [TH, TW]: the render pixel of every display pixel."""
    Y, X = np.mgrid[0:TH, 0:TW].astype(np.int64)
    return np.minimum(h - 1, ((2 * Y + 1) * h) // (2 * TH)), np.minimum(w - 1, ((2 * X + 1) * w) // (2 * TW))


def _project(cam, pos, P, TW, TH):
    R0, R1, R2, det = cam
    d = P - _v3(pos)
    a, b, l = _dot3(d, R0), _dot3(d, R1), _dot3(d, R2)
    front = np.isfinite(l) & (l != 0) & ((l > 0) == bool(det > 0))
    sx, sy = a / l, b / l
    return front, ((sx + F(1.0)) * F(0.5)) * F(TW) - F(0.5), ((sy + F(1.0)) * F(0.5)) * F(TH) - F(0.5)


def alpha_of(ux, uy, X, Y):
    """The sample weight in 1/256 of a sample at (ux, uy) for pixel (X, Y), arrays of float32."""
    with np.errstate(all="ignore"):
        dx, dy = np.abs(ux - X), np.abs(uy - Y)
        m = np.fmax(dx, dy)
        near = (dx < F(1.0)) & (dy < F(1.0))
        return np.where(near, 256 - np.floor(np.where(near, m, F(0)) * F(256.0)).astype(np.int64), 0).astype(np.uint64)


def blend(h, c, a, n):
    """(h (256 n - a) + (c << 8) a + 128 n) / (256 n) in integers; the numerator must fit 32 bits."""
    h, c, a, n = (np.asarray(v, np.uint64) for v in (h, c, a, n))
    num = h * (256 * n - a) + (c * 256) * a + 128 * n
    assert (num < (1 << 32)).all()
    return num // (256 * n)


def upsample(w, h, TW, TH, cur, prev, color8, position, normal8, hist=None, max_history=32, tol_abs=0.5, tol_rel=None):
    """One frame.  color8 uint8 [h, w, 4], position float32 [h, w, 4], normal8 int8 [h, w, 4]; hist: the previous frame's
    (color16, surface) at TW x TH or None.  Returns a dict: color16, surface, resolved8 uint8 [TH, TW, 4], motion float32
    [TH, TW, 2], cls (index into CLASSES, by the taps), alpha (the sample weight, 256 where none is computed), weight (the sum of
    the valid taps' weights) and copied (the pixel carried the nearest history texel whole) of every display pixel."""
    assert 1 <= max_history <= 255 and TW >= w and TH >= h
    kc, kp = camera(w, h, cur), camera(w, h, prev)
    assert kc is not None and kp is not None, "degenerate basis"
    tol_abs = F(tol_abs)
    tol_rel = default_tol_rel(cur, w) if tol_rel is None else F(tol_rel)
    ry, rx = source(w, h, TW, TH)
    c = np.ascontiguousarray(color8).reshape(h, w, 4)[ry, rx].astype(np.uint64)
    pos_bits = np.ascontiguousarray(position, dtype=F).reshape(h, w, 4).view(np.uint32)[ry, rx]
    P = pos_bits.view(F)[..., :3]
    N = np.ascontiguousarray(normal8).reshape(h, w, 4).view(np.uint8).astype(np.uint32)[ry, rx]
    N = N[..., 0] | (N[..., 1] << 8) | (N[..., 2] << 16) | (N[..., 3] << 24)
    nbits = N & np.uint32(0xFFFFFF)
    miss = N == 0
    Yi, Xi = np.mgrid[0:TH, 0:TW]
    X, Y = Xi.astype(F), Yi.astype(F)
    with np.errstate(all="ignore"):
        fc, ux, uy = _project(kc, cur.cam_pos, P, TW, TH)
        ux, uy = np.where(fc, ux, X), np.where(fc, uy, Y)
        alpha = np.where(fc, alpha_of(ux, uy, X, Y), 256).astype(np.uint64)
        front, vx, vy = _project(kp, prev.cam_pos, P, TW, TH)
        front &= ~miss
        mvx, mvy = vx - ux, vy - uy
        motion = np.zeros((TH, TW, 2), F)
        motion[..., 0] = np.where(front, mvx, F(0))
        motion[..., 1] = np.where(front, mvy, F(0))
        qx, qy = X + mvx, Y + mvy
        taps = front & np.isfinite(qx) & np.isfinite(qy)
        if hist is None:
            taps = np.zeros_like(taps)
        x0f, y0f = np.floor(qx), np.floor(qy)
        wx = np.where(taps, np.floor((qx - x0f) * F(256.0) + F(0.5)), 0).astype(np.int64)
        wy = np.where(taps, np.floor((qy - y0f) * F(256.0) + F(0.5)), 0).astype(np.int64)
        x0 = np.where(taps, np.clip(x0f, F(-2.0), F(TW)), 0).astype(np.int64)
        y0 = np.where(taps, np.clip(y0f, F(-2.0), F(TH)), 0).astype(np.int64)
        dc = P - _v3(cur.cam_pos)
        tol = tol_abs + tol_rel * np.sqrt(_dot3(dc, dc))
        tol2 = tol * tol
        ws = np.zeros((TH, TW), np.uint64)
        acc = np.zeros((TH, TW, 4), np.uint64)
        cmin = np.full((TH, TW), 255, np.uint64)
        nonzero = np.zeros((TH, TW), np.int64)
        nvalid = np.zeros((TH, TW), np.int64)
        inside_any = np.zeros((TH, TW), bool)
        if hist is not None:
            h16 = np.ascontiguousarray(hist[0]).reshape(TH, TW, 4).astype(np.uint64)
            hs = np.ascontiguousarray(hist[1]).reshape(TH, TW, 4).view(np.uint32)
            hpos = hs.view(F)[..., :3]
            for t in range(4):
                tx, ty = x0 + (t & 1), y0 + (t >> 1)
                wt = (wx if t & 1 else 256 - wx) * (wy if t >> 1 else 256 - wy)
                live = taps & (wt != 0)
                inside = live & (tx >= 0) & (tx < TW) & (ty >= 0) & (ty < TH)
                txc, tyc = np.clip(tx, 0, TW - 1), np.clip(ty, 0, TH - 1)
                s = hs[tyc, txc]
                e = hpos[tyc, txc] - P
                ok = inside & ((s[..., 3] & np.uint32(0xFFFFFF)) == nbits) & (_dot3(e, e) <= tol2)
                wv = np.where(ok, wt, 0).astype(np.uint64)
                ws += wv
                acc += wv[..., None] * h16[tyc, txc]
                cmin = np.where(ok, np.minimum(cmin, (s[..., 3] >> 24).astype(np.uint64)), cmin)
                nonzero += live; nvalid += ok; inside_any |= inside
    has = ws != 0
    wsd = np.where(has, ws, 1)
    hh = (acc + (ws // 2)[..., None]) // wsd[..., None]
    n = np.where(has, np.minimum(cmin + 1, np.uint64(max_history)), 1).astype(np.uint64)
    blended = blend(np.where(has[..., None], hh, 0), c, np.where(has, alpha, 0)[..., None], n[..., None])
    color16 = np.where(has[..., None], blended, c * 256)
    surface = np.zeros((TH, TW, 4), np.uint32)
    surface[..., :3] = np.where(miss[..., None], np.uint32(0), pos_bits[..., :3])
    surface[..., 3] = np.where(miss, np.uint32(1 << 24), nbits | (n.astype(np.uint32) << 24))
    # a pixel no sample fell on (alpha 0) whose far sample matches no tap carries the history texel nearest to q, whole
    nx, ny = x0 + (wx >= 128), y0 + (wy >= 128)
    copied = taps & ~has & (alpha == 0) & (nx >= 0) & (nx < TW) & (ny >= 0) & (ny < TH)
    if hist is not None:
        nxc, nyc = np.clip(nx, 0, TW - 1), np.clip(ny, 0, TH - 1)
        color16 = np.where(copied[..., None], h16[nyc, nxc], color16)
        surface = np.where(copied[..., None], hs[nyc, nxc], surface)
    resolved = np.minimum((color16 + 128) >> 8, 255).astype(np.uint8)
    cls = np.full((TH, TW), 3, np.uint8)                                # disoccluded: a hit without a valid tap
    cls[~miss & ~front] = 5
    cls[taps & ~inside_any] = 4
    cls[front & ~taps & (hist is not None)] = 4                         # projected to infinity
    cls[has & (nvalid < nonzero)] = 2
    cls[has & (nvalid == nonzero)] = 1
    cls[miss] = 0
    return {"color16": color16.astype(np.uint16), "surface": surface, "resolved8": resolved, "motion": motion, "cls": cls,
            "alpha": np.where(miss, 256, alpha).astype(np.uint16), "weight": ws, "copied": copied}


def shares(cls, alpha):
    """Share of every class among all pixels, and of the pixels with history (full or partial) whose sample counted (alpha > 0:
    sampled) or did not (alpha == 0: carried), also among all pixels."""
    out = {name: float((cls == k).mean()) for k, name in enumerate(CLASSES)}
    has = (cls == 1) | (cls == 2)
    out["sampled"] = float((has & (alpha > 0)).mean())
    out["carried"] = float((has & (alpha == 0)).mean())
    return out
