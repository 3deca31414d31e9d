"""Temporal upsampling for ray cameras, the definition restated in numpy: every fp32 step of csrc/vrt_upsample_cam.h (and of the
vrt_spec.h functions it calls, through tests/reproject_cam_reference.py) as one float32 array operation, every integer step in
uint64; and camera_ray_offset / panorama_tables_offset of csrc/vrt_raygen.h the same way (the host's double-precision parts in
Python floats).  Shares no code with the headers; tests/test_upsample_cam_cpu.py and tests/test_raygen_offset_cpu.py compare the
two bit for bit, tests/test_gpu_upsample_cam.py the kernels against this.

A camera is anything with model / basis (cam_pos, cam_dir, cam_right, cam_up) / tan_half / half_width: the package's
_capi.RayCamera.  The frame is w x h, the history (color16 uint16 [TH, TW, 4], surface uint32 [TH, TW, 4]) and every output
TW x TH."""
import math

import numpy as np

import reproject_cam_reference as rcr
from reproject_cam_reference import KU, KV, ORTHOGRAPHIC, PANORAMA, PERSPECTIVE, _basis, _normalize, asin_spec, atan2_spec, default_tol_rel  # noqa: F401
from reproject_reference import _cross, _dot3, _v3, same  # noqa: F401  (same: re-exported)
from upsample_reference import blend, source

F = np.float32


# ---- rays with a sub-pixel offset (csrc/vrt_raygen.h: camera_ray_offset) -------------------------------------------------------

def panorama_tables_offset(W, H, ox, oy):
    ku, kv = float(KU), float(KV)
    ox, oy = float(F(ox)), float(F(oy))
    th = [(((px + 0.5) + ox) / W - 0.5) / ku for px in range(W)]
    ph = [(((py + 0.5) + oy) / H - 0.5) / kv for py in range(H)]
    col = np.array([[math.cos(t), math.sin(t)] for t in th], np.float64).astype(F)
    row = np.array([[math.cos(p), math.sin(p)] for p in ph], np.float64).astype(F)
    return col, row


def camera_rays_offset(cam, W, H, offset):
    """(origins, dirs), each (H * W, 3) float32, ray py * W + px through (px + 0.5 + ox, py + 0.5 + oy)."""
    ox, oy = F(offset[0]), F(offset[1])
    pos = _v3(cam.basis.cam_pos)
    if cam.model == PANORAMA:
        col, row = panorama_tables_offset(W, H, ox, oy)
        ct, st = col[None, :, 0], col[None, :, 1]
        cp, sp = row[:, None, 0], row[:, None, 1]
        d = np.stack([cp * ct, np.broadcast_to(-sp, (H, W)), cp * st], axis=-1).astype(F)
        o = np.broadcast_to(pos, (H, W, 3)).astype(F)
        return o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    cd, U, V, jx, jy = _basis(cam, W, H)
    sx = ((((np.arange(W, dtype=F) + F(0.5)) + ox) / F(W)) * F(2) - F(1)).astype(F)[None, :, None]
    sy = ((((np.arange(H, dtype=F) + F(0.5)) + oy) / F(H)) * F(2) - F(1)).astype(F)[:, None, None]
    if cam.model == ORTHOGRAPHIC:
        o = ((pos + sx * U) + sy * V).astype(F)
        d = np.broadcast_to(cd, (H, W, 3)).astype(F)
        return o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    J = np.array([jx, jy, F(0)], F)
    v = (((cd + sx * U) + sy * V) + J).astype(F)
    o = np.broadcast_to(pos, (H, W, 3)).astype(F)
    return o.reshape(-1, 3).copy(), _normalize(v).reshape(-1, 3).copy()


# ---- the pass (csrc/vrt_upsample_cam.h) -----------------------------------------------------------------------------------------

def camera(w, h, cam):
    """R0, R1, R2, det of cam without jitter and offset (zeros for a panorama; None: degenerate in fp32)."""
    if cam.model == PANORAMA:
        z = np.zeros(3, F)
        return z, z, z, F(0.0)
    with np.errstate(all="ignore"):
        cd, U, V, _, _ = _basis(cam, w, h)
        R0, R1, R2 = _cross(V, cd), _cross(cd, U), _cross(U, V)
        det = _dot3(U, R0)
    if not np.isfinite(det) or det == 0:
        return None
    return R0, R1, R2, det


def project(w, h, TW, TH, cam, P):
    """(front, x, y) of world points P [..., 3] on the TW x TH grid through cam; x, y are meaningless where front is False."""
    R0, R1, R2, det = camera(w, h, cam)
    with np.errstate(all="ignore"):
        d = (P - _v3(cam.basis.cam_pos)).astype(F)
        if cam.model == PANORAMA:
            front = np.isfinite(d).all(axis=-1) & ~(d == 0).all(axis=-1)
            u = atan2_spec(d[..., 2], d[..., 0]) * KU + F(0.5)
            t = asin_spec(-_normalize(d)[..., 1]) * KV + F(0.5)
            x = u * F(TW) - F(0.5)
            y = t * F(TH) - F(0.5)
        else:
            a, b, l = _dot3(d, R0), _dot3(d, R1), _dot3(d, R2)
            front = np.isfinite(l) & (l != 0) & ((l > 0) == bool(det > 0))
            den = det if cam.model == ORTHOGRAPHIC else l
            sx, sy = a / den, b / den
            x = ((sx + F(1.0)) * F(0.5)) * F(TW) - F(0.5)
            y = ((sy + F(1.0)) * F(0.5)) * F(TH) - F(0.5)
    return front, x.astype(F), y.astype(F)


def alpha_of(model, ux, uy, X, Y, TW):
    """The sample weight in 1/256; the panorama's x distance the short way round (S1)."""
    with np.errstate(all="ignore"):
        dx, dy = np.abs(ux - X), np.abs(uy - Y)
        if model == PANORAMA:
            dx = np.fmin(dx, F(TW) - dx)
        m = np.fmax(dx, dy)
        near = (dx < F(1.0)) & (dy < F(1.0))
        return np.where(near, 256 - np.floor(np.where(near, m, F(0)) * F(256.0)).astype(np.int64), 0).astype(np.uint64)


def _wrap(model, tx, TW):
    return np.where(tx < 0, tx + TW, np.where(tx >= TW, tx - TW, tx)) if model == PANORAMA else tx


def upsample(w, h, TW, TH, cur, prev, color8, position, normal8, hist=None, max_history=32, tol_abs=0.5, tol_rel=None):
    """One frame.  color8 uint8 [h, w, 4], position float32 [h, w, 4], normal8 int8 [h, w, 4]; hist: the previous frame's
    (color16, surface) at TW x TH or None.  Returns a dict: color16, surface, resolved8 uint8 [TH, TW, 4], motion float32
    [TH, TW, 2], and of every display pixel ux (where its sample fell, x), alpha (the sample weight, 256 where none is computed),
    seam_alpha (the weight is non-zero only by S1), wrapped (a valid tap, or the carried texel, came through the wrap S3 / S4)
    and copied (it carried the nearest history texel whole)."""
    assert 1 <= max_history <= 255 and TW >= w and TH >= h and cur.model == prev.model
    model = cur.model
    assert camera(w, h, cur) is not None and camera(w, h, prev) is not None, "degenerate basis"
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
        fc, ux, uy = project(w, h, TW, TH, cur, P)
        ux, uy = np.where(fc, ux, X), np.where(fc, uy, Y)
        alpha = np.where(fc, alpha_of(model, ux, uy, X, Y, TW), 256).astype(np.uint64)
        seam_alpha = fc & ~miss & (alpha != 0) & ~(np.abs(ux - X) < F(1.0))
        front, vx, vy = project(w, h, TW, TH, prev, P)
        front &= ~miss
        mvx, mvy = (vx - ux).astype(F), (vy - uy).astype(F)
        motion = np.zeros((TH, TW, 2), F)
        motion[..., 0] = np.where(front, mvx, F(0))
        motion[..., 1] = np.where(front, mvy, F(0))
        qx0, qy = (X + mvx).astype(F), (Y + mvy).astype(F)
        qx = qx0
        if model == PANORAMA:                                                # S3
            qx = np.where(qx0 < F(-0.5), qx0 + F(TW), np.where(qx0 >= F(TW) - F(0.5), qx0 - F(TW), qx0)).astype(F)
        shifted = qx != qx0
        taps = front & np.isfinite(qx) & np.isfinite(qy)
        if hist is None:
            taps = np.zeros_like(taps)
        x0f, y0f = np.floor(qx), np.floor(qy)
        wx = np.where(taps, np.floor((qx - x0f) * F(256.0) + F(0.5)), 0).astype(np.int64)
        wy = np.where(taps, np.floor((qy - y0f) * F(256.0) + F(0.5)), 0).astype(np.int64)
        x0 = np.where(taps, np.clip(x0f, F(-2.0), F(TW)), 0).astype(np.int64)
        y0 = np.where(taps, np.clip(y0f, F(-2.0), F(TH)), 0).astype(np.int64)
        if model == ORTHOGRAPHIC:
            tol = np.broadcast_to(tol_abs + tol_rel, (TH, TW))
        else:
            dc = P - _v3(cur.basis.cam_pos)
            tol = tol_abs + tol_rel * np.sqrt(_dot3(dc, dc))
        tol2 = (tol * tol).astype(F)
        ws = np.zeros((TH, TW), np.uint64)
        acc = np.zeros((TH, TW, 4), np.uint64)
        cmin = np.full((TH, TW), 255, np.uint64)
        wrapped = np.zeros((TH, TW), bool)
        if hist is not None:
            h16 = np.ascontiguousarray(hist[0]).reshape(TH, TW, 4).astype(np.uint64)
            hs = np.ascontiguousarray(hist[1]).reshape(TH, TW, 4).view(np.uint32)
            hpos = hs.view(F)[..., :3]
            for t in range(4):
                tx0, ty = x0 + (t & 1), y0 + (t >> 1)
                tx = _wrap(model, tx0, TW)                                   # S4
                wt = (wx if t & 1 else 256 - wx) * (wy if t >> 1 else 256 - wy)
                inside = taps & (wt != 0) & (tx >= 0) & (tx < TW) & (ty >= 0) & (ty < TH)
                txc, tyc = np.clip(tx, 0, TW - 1), np.clip(ty, 0, TH - 1)
                s = hs[tyc, txc]
                e = hpos[tyc, txc] - P
                ok = inside & ((s[..., 3] & np.uint32(0xFFFFFF)) == nbits) & (_dot3(e, e) <= tol2)
                wv = np.where(ok, wt, 0).astype(np.uint64)
                ws += wv
                acc += wv[..., None] * h16[tyc, txc]
                cmin = np.where(ok, np.minimum(cmin, (s[..., 3] >> 24).astype(np.uint64)), cmin)
                wrapped |= ok & ((tx != tx0) | shifted)
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
    nx0, ny = x0 + (wx >= 128), y0 + (wy >= 128)
    nx = _wrap(model, nx0, TW)
    copied = taps & ~has & (alpha == 0) & (nx >= 0) & (nx < TW) & (ny >= 0) & (ny < TH)
    if hist is not None:
        nxc, nyc = np.clip(nx, 0, TW - 1), np.clip(ny, 0, TH - 1)
        color16 = np.where(copied[..., None], h16[nyc, nxc], color16)
        surface = np.where(copied[..., None], hs[nyc, nxc], surface)
        wrapped |= copied & ((nx != nx0) | shifted)
    # a miss writes its nearest sample (step 2), whatever the rest computed
    color16 = np.where(miss[..., None], c * 256, color16)
    surface[miss] = np.array([0, 0, 0, 1 << 24], np.uint32)
    motion[miss] = 0
    resolved = np.minimum((color16 + 128) >> 8, 255).astype(np.uint8)
    return {"color16": color16.astype(np.uint16), "surface": surface, "resolved8": resolved, "motion": motion,
            "ux": np.where(miss, X, ux).astype(F), "alpha": np.where(miss, 256, alpha).astype(np.uint16),
            "seam_alpha": seam_alpha, "wrapped": wrapped & ~miss, "copied": copied & ~miss}
