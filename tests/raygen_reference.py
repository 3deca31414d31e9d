"""numpy float32 restatement of csrc/vrt_raygen.h, the definition of vrt_camera_rays' three camera models: every operation in
the header's order, one rounding per operation (numpy float32 arithmetic does not contract), the host's double-precision parts
in Python floats.  Shares no code with the header; tests/test_raygen_cpu.py holds the two to bit equality."""
import math

import numpy as np

PERSPECTIVE, ORTHOGRAPHIC, PANORAMA = 0, 1, 2
F = np.float32


def _normalize(v):
    v = np.asarray(v, F)
    l = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        out = v / l[..., None]
    return np.where((l == 0)[..., None], F(0), out).astype(F)


def screen(W, H):
    """sx (W,), sy (H,): ((p + 0.5) / N) * 2 - 1"""
    sx = ((np.arange(W, dtype=F) + F(0.5)) / F(W)) * F(2) - F(1)
    sy = ((np.arange(H, dtype=F) + F(0.5)) / F(H)) * F(2) - F(1)
    return sx.astype(F), sy.astype(F)


def panorama_tables(W, H):
    ku, kv = float(F(0.1591)), float(F(0.3183))
    th = [((px + 0.5) / W - 0.5) / ku for px in range(W)]
    ph = [((py + 0.5) / H - 0.5) / kv for py in range(H)]
    col = np.array([[math.cos(t), math.sin(t)] for t in th], np.float64).astype(F)
    row = np.array([[math.cos(p), math.sin(p)] for p in ph], np.float64).astype(F)
    return col, row


def camera_rays(model, W, H, pos, cam_dir=(0, 0, 1), right=(1, 0, 0), up=(0, -1, 0), jitter=(0, 0), tan_half=1.0, half_width=1.0):
    """(origins, dirs), each (H * W, 3) float32, ray py * W + px for pixel (px, py)."""
    pos = np.asarray(pos, F)
    if model == PANORAMA:
        col, row = panorama_tables(W, H)
        ct, st = col[None, :, 0], col[None, :, 1]
        cp, sp = row[:, None, 0], row[:, None, 1]
        d = np.stack([cp * ct, np.broadcast_to(-sp, (H, W)), cp * st], axis=-1).astype(F)
        o = np.broadcast_to(pos, (H, W, 3)).astype(F)
        return o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    scale = F(tan_half if model == PERSPECTIVE else half_width)
    cd = _normalize(np.asarray(cam_dir, F))
    U = (np.asarray(right, F) * scale).astype(F)
    V = (((np.asarray(up, F) * scale) * F(H)) / F(W)).astype(F)
    sx, sy = screen(W, H)
    sx, sy = sx[None, :, None], sy[:, None, None]
    if model == ORTHOGRAPHIC:
        o = ((pos + sx * U) + sy * V).astype(F)
        d = np.broadcast_to(cd, (H, W, 3)).astype(F)
        return o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
    J = np.array([(F(jitter[0]) / F(W)) * F(-2), (F(jitter[1]) / F(H)) * F(2), F(0)], F)
    v = (((cd + sx * U) + sy * V) + J).astype(F)
    d = _normalize(v)
    o = np.broadcast_to(pos, (H, W, 3)).astype(F)
    return o.reshape(-1, 3).copy(), d.reshape(-1, 3).copy()
