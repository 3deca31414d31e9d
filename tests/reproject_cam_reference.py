"""Temporal reprojection for ray cameras, the definition restated in numpy: every fp32 step of csrc/vrt_reproject_cam.h (and of
the vrt_spec.h functions it calls: atan2_spec, asin_spec, normalize3) as one float32 array operation, every integer step in
uint64.  Shares no code with the headers; tests/test_reproject_cam_cpu.py compares the two bit for bit,
tests/test_gpu_reproject_cam.py the kernel against this.

A camera is anything with model / basis (cam_pos, cam_dir, cam_right, cam_up, camera_jitter) / tan_half / half_width: the
package's _capi.RayCamera.  A history is (color16 uint16 [H, W, 4], surface uint32 [H, W, 4])."""
import numpy as np

from reproject_reference import _cross, _dot3, _v3, same, shares  # noqa: F401  (vector helpers and the plane comparison)

F = np.float32
PERSPECTIVE, ORTHOGRAPHIC, PANORAMA = 0, 1, 2
CLASSES = ("miss", "full", "partial", "disoccluded", "outside", "behind")
KU, KV = F(0.1591), F(0.3183)
PI, PI_2, PI_4 = F(3.14159265358979323846), F(1.57079632679489661923), F(0.78539816339744830962)


def _normalize(v):
    l = np.sqrt(_dot3(v, v))
    with np.errstate(all="ignore"):
        out = v / l[..., None]
    return np.where((l == 0)[..., None], F(0), out).astype(F)


def atan_unit(t):
    t = np.asarray(t, F)
    red = t > F(0.4142135623730950)
    with np.errstate(all="ignore"):
        q = (t - F(1.0)) / (t + F(1.0))
    y0 = np.where(red, PI_4, F(0.0)).astype(F)
    t = np.where(red, q, t).astype(F)
    z = t * t
    p = (((F(8.05374449538e-2) * z - F(1.38776856032e-1)) * z + F(1.99777106478e-1)) * z - F(3.33329491539e-1)) * z * t + t
    return (p + y0).astype(F)


def atan2_spec(y, x):
    y, x = np.asarray(y, F), np.asarray(x, F)
    ax, ay = np.abs(x), np.abs(y)
    zero = (ax == 0) & (ay == 0)
    swap = ay > ax
    with np.errstate(all="ignore"):
        t = np.where(swap, ax, ay) / np.where(swap, ay, ax)
    r = atan_unit(t)
    r = np.where(swap, PI_2 - r, r).astype(F)
    r = np.where(x < 0, PI - r, r).astype(F)
    r = np.where(y < 0, -r, r).astype(F)
    return np.where(zero, F(0.0), r).astype(F)


def asin_spec(x):
    x = np.asarray(x, F)
    a = np.abs(x)
    big = a > F(0.5)
    a = np.where(a > F(1.0), F(1.0), a).astype(F)
    with np.errstate(all="ignore"):
        zb = F(0.5) * (F(1.0) - a)
        sb = np.sqrt(zb)
    z = np.where(big, zb, a * a).astype(F)
    s = np.where(big, sb, a).astype(F)
    p = ((((F(4.2163199048e-2) * z + F(2.4181311049e-2)) * z + F(4.5470025998e-2)) * z + F(7.4953002686e-2)) * z + F(1.6666752422e-1)) * z * s + s
    p = np.where(big, PI_2 - (p + p), p).astype(F)
    return np.where(x < 0, -p, p).astype(F)


def _basis(cam, W, H):
    """(cd, U, V, jx, jy) as raygen_consts_of builds them."""
    b = cam.basis
    scale = F(cam.tan_half if cam.model == PERSPECTIVE else cam.half_width)
    cd = _normalize(_v3(b.cam_dir))
    U = (_v3(b.cam_right) * scale).astype(F)
    V = (((_v3(b.cam_up) * scale) * F(H)) / F(W)).astype(F)
    jx = jy = F(0.0)
    if cam.model == PERSPECTIVE:
        jx = (F(b.camera_jitter[0]) / F(W)) * F(-2.0)
        jy = (F(b.camera_jitter[1]) / F(H)) * F(2.0)
    return cd, U, V, jx, jy


def default_tol_rel(cur, W):
    if cur.model == PANORAMA:
        return F(2.0) / (KU * F(W))
    _, U, _, _, _ = _basis(cur, W, 1)
    return (F(4.0) * np.sqrt(_dot3(U, U))) / F(W)


def consts(W, H, prev):
    """R0, R1, R2, det of the previous camera (zeros for a panorama; None: degenerate)."""
    if prev.model == PANORAMA:
        z = np.zeros(3, F)
        return z, z, z, F(0.0)
    with np.errstate(all="ignore"):
        cd, U, V, jx, jy = _basis(prev, W, H)
        Co = np.array([cd[0] + jx, cd[1] + jy, cd[2]], F) if prev.model == PERSPECTIVE else cd
        R0, R1, R2 = _cross(V, Co), _cross(Co, U), _cross(U, V)
        det = _dot3(U, R0)
    if not np.isfinite(det) or det == 0:
        return None
    return R0, R1, R2, det


def project(W, H, prev, P):
    """(front, qx, qy) of world points P [..., 3] on prev's screen; qx, qy are meaningless where front is False."""
    model = prev.model
    R0, R1, R2, det = consts(W, H, prev)
    with np.errstate(all="ignore"):
        d = (P - _v3(prev.basis.cam_pos)).astype(F)
        if model == PANORAMA:
            front = np.isfinite(d).all(axis=-1) & ~(d == 0).all(axis=-1)
            u = atan2_spec(d[..., 2], d[..., 0]) * KU + F(0.5)
            t = asin_spec(-_normalize(d)[..., 1]) * KV + F(0.5)
            qx = u * F(W) - F(0.5)
            qy = t * F(H) - F(0.5)
        else:
            a, b, l = _dot3(d, R0), _dot3(d, R1), _dot3(d, R2)
            front = np.isfinite(l) & (l != 0) & ((l > 0) == bool(det > 0))
            den = det if model == ORTHOGRAPHIC else l
            sx, sy = a / den, b / den
            qx = ((sx + F(1.0)) * F(0.5)) * F(W) - F(0.5)
            qy = ((sy + F(1.0)) * F(0.5)) * F(H) - F(0.5)
    return front, qx.astype(F), qy.astype(F)


def reproject(W, H, cur, prev, color8, position, normal8, hist=None, max_history=32, tol_abs=0.5, tol_rel=None):
    """One frame.  color8 uint8 [H, W, 4], position float32 [H, W, 4], normal8 int8 [H, W, 4]; hist: the previous frame's
    (color16, surface) or None.  Returns a dict: color16, surface, resolved8, motion float32 [H, W, 2], cls (index into CLASSES)
    and wrapped (bool [H, W]: a tap of non-zero weight was taken from the other end of its row)."""
    assert 1 <= max_history <= 255 and cur.model == prev.model
    model = prev.model
    assert consts(W, H, prev) is not None, "degenerate basis"
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
        front, qx, qy = project(W, H, prev, P)
        front = front & ~miss
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
        if model == ORTHOGRAPHIC:
            tol = np.broadcast_to(tol_abs + tol_rel, (H, W))
        else:
            dc = P - _v3(cur.basis.cam_pos)
            tol = tol_abs + tol_rel * np.sqrt(_dot3(dc, dc))
        tol2 = (tol * tol).astype(F)
        ws = np.zeros((H, W), np.uint64)
        acc = np.zeros((H, W, 4), np.uint64)
        cmin = np.full((H, W), 255, np.uint64)
        nonzero = np.zeros((H, W), np.int64)
        nvalid = np.zeros((H, W), np.int64)
        inside_any = np.zeros((H, W), bool)
        wrapped = np.zeros((H, W), bool)
        if hist is not None:
            h16 = np.ascontiguousarray(hist[0]).reshape(H, W, 4).astype(np.uint64)
            hs = np.ascontiguousarray(hist[1]).reshape(H, W, 4).view(np.uint32)
            hpos = hs.view(F)[..., :3]
            for t in range(4):
                tx, ty = x0 + (t & 1), y0 + (t >> 1)
                w = (wx if t & 1 else 256 - wx) * (wy if t >> 1 else 256 - wy)
                live = taps & (w != 0)
                if model == PANORAMA:
                    tw = np.where(tx < 0, tx + W, np.where(tx >= W, tx - W, tx))
                    wrapped |= live & (tw != tx) & (tw >= 0) & (tw < W) & (ty >= 0) & (ty < H)
                    tx = tw
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
    return {"color16": color16.astype(np.uint16), "surface": surface, "resolved8": resolved, "motion": motion, "cls": cls,
            "wrapped": wrapped}
