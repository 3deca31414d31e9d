"""Volumes, ray batches and cameras at the documented size limits (include/vrt.h: 1..4096 voxels, 1..512 bricks per axis), shared by
tests/test_extents_cpu.py (host builds against the oracle, and the batches' and cameras' composition on the oracle alone) and
tests/test_gpu_extents.py.
  needles        4096 (ragged: 4093) voxels along one axis, 5 x 6 across: cell coordinates 0 .. 1023 of the occupied-cell list, the last
                 value that fits its 10 bits;
  brick needles  512 bricks along one axis, one across (4096 x 8 x 8 voxels): brick coordinates 0 .. 511;
  slabs          (W + 2)(H + 2) on either side of 2^23, three slices deep: the largest slice the look-up loops (vrt_march_fast.h) and
                 the 32-bit / 24-bit-multiply form of VRT_TRAVERSAL_DF (vrt_march_df.h, df_small) may take, and the first they must
                 refuse."""
import numpy as np

from ray_query_common import long_rays

NEEDLES = [(4096, 5, 6), (5, 4096, 6), (6, 5, 4096)]
RAGGED = [(4093, 5, 6), (5, 4093, 6), (6, 5, 4093)]              # the last 4^3 and 64^3 cells are partial
BRICK_NEEDLES = [(512, 1, 1), (1, 512, 1), (1, 1, 512)]           # bricks; 4096 x 8 x 8 voxels
LINES = [(4096, 1, 1), (1, 4096, 1), (1, 1, 4096)]                 # (scene build and its definition only)
# (W + 2)(H + 2) = 2^23 - 4096: the largest slice df_fast_layout_ok and df_small accept; exactly 2^23: the first they refuse
SLABS = [((4094, 2045, 3), True), ((4094, 2046, 3), False), ((2045, 4094, 3), True), ((2046, 4094, 3), False)]
BUDGETS = (1024, 1025, 5000)          # VRT_TRAVERSAL_AUTO: the look-up loop up to 1024, the general march from 1025 on; needles and slabs alike
N_RAYS = 1000
FRAMES = [(96, 64), (45, 37)]
METAL = 230                            # an id of helpers.metallic_palette's metallic range


def long_axis(dims):
    return int(np.argmax(dims))


def needle_volume(dims):
    """[z, y, x] of a W x H x D needle.  Along the long axis, from either end: a solid cap three voxels deep; single voxels with
    p = 0.01 over the 23 voxels next to the cap and p = 0.002 over the next 64 (a ray along the axis passes both ends' stretches
    with probability 0.5; a needle this dense all along would let none see the far end); the middle 64 voxels at p = 0.002; empty in
    between, so that the clearances reach their cap, but for a ledge one voxel high along one side, 600 voxels past the middle
    (what the camera in the middle sees within 1024 steps; a ray along the axis passes beside it).  The eight corner voxels carry ids of their own, one of them metallic:
    cell coordinate 0 and the last one are occupied on the long axis whatever the caps hold."""
    W, H, D = dims
    a = long_axis(dims)
    L = dims[a]
    rng = np.random.default_rng(W * 1000003 + H * 1009 + D)
    vol = np.zeros((D, H, W), np.uint8)
    p = np.zeros(L)
    p[3:26] = 0.01; p[26:90] = 0.002; p[L - 26:L - 3] = 0.01; p[L - 90:L - 26] = 0.002; p[L // 2 - 32:L // 2 + 32] = 0.002
    shape = [1, 1, 1]; shape[2 - a] = L
    vol[...] = (rng.random((D, H, W)) < p.reshape(shape)) * rng.integers(1, 256, (D, H, W))
    cap = [slice(None)] * 3
    cap[2 - a] = slice(0, 3); vol[tuple(cap)] = 9
    cap[2 - a] = slice(L - 3, L); vol[tuple(cap)] = 11
    ledge = [slice(None)] * 3
    ledge[2 - a] = slice(L // 2 + 600, L // 2 + 602); ledge[2 - [b for b in range(3) if b != a][0]] = 0
    vol[tuple(ledge)] = 15
    for k in range(8):
        vol[(D - 1) * (k >> 2), (H - 1) * (k >> 1 & 1), (W - 1) * (k & 1)] = METAL if k == 7 else 20 + k
    return vol


def brick_needle_volume(nb):
    """needle_volume's content over nb[0] * 8 x nb[1] * 8 x nb[2] * 8 voxels"""
    return needle_volume(tuple(8 * n for n in nb))


def needle_rays(dims, sign, n=N_RAYS):
    """n rays nearly parallel to the long axis of a needle, towards its far end (sign > 0: the high one).  A fifth starts
    just outside the near face, two fifths behind the near cap (within 60 voxels), a fifth in the middle and a fifth within 100
    voxels of the far end; seven in ten
    have a slope of at most 0.0002 against the axis (from the middle of the section they stay inside for the whole length), the
    others up to 0.05 (they leave through a side)."""
    a = long_axis(dims)
    L = dims[a]
    fifth = [(-3.0, 0.5), (2.5, 60.0), (2.5, 60.0), (L / 2 - 40.0, L / 2 + 40.0), (L - 100.0, L - 3.0)]
    return long_rays(n, dims=dims, axis=a, sign=sign, along=fifth, margin=2.0, slopes=(0.0002, 0.05), seed=4096 + 2 * a + (sign > 0))


def slab_volume(dims):
    """[z, y, x]: single voxels with p = 0.0004 (a ray passes 2000 voxels with probability 0.45), with p = 0.02 within 150 voxels
    of the far corner in x and y (what the cameras look at), and a solid 3 x 3 block at the highest x and y of every slice, one
    voxel of it metallic"""
    W, H, D = dims
    rng = np.random.default_rng(W * 1000003 + H * 1009 + D)
    p = np.full((H, W), 0.0004); p[H - 150:, W - 150:] = 0.02
    vol = ((rng.random((D, H, W)) < p[None]) * rng.integers(1, 200, (D, H, W))).astype(np.uint8)
    vol[:, H - 3:, W - 3:] = 13
    vol[:, H - 1, W - 1] = METAL
    return vol


def slab_rays(dims, n=N_RAYS):
    """n rays inside a slab: from within 40 voxels of one of its four corners (in x and y; ray i from corner i % 4) along x, along
    y or along the diagonal (i // 4 % 3), towards the opposite side; from the middle slice with a z slope of +-(0.002 .. 0.004) per
    voxel travelled (the sign by i // 12 % 2), so that a ray changes slice after 125 .. 500 voxels -- towards z = 2 or towards z = 0 -- and
    leaves the slab after at most 1000."""
    W, H, D = dims
    assert D == 3
    rng = np.random.default_rng(W * 31 + H)
    i = np.arange(n)
    cx, cy = (i % 4) & 1, (i % 4) >> 1
    o = np.stack([np.where(cx, W - rng.uniform(0.5, 40.0, n), rng.uniform(0.5, 40.0, n)),
                  np.where(cy, H - rng.uniform(0.5, 40.0, n), rng.uniform(0.5, 40.0, n)), rng.uniform(1.25, 1.75, n)], axis=1)
    kind = i // 4 % 3
    sx, sy = np.where(cx, -1.0, 1.0), np.where(cy, -1.0, 1.0)
    wobble = rng.uniform(0.0005, 0.01, n)                          # (away from the wall the origin is next to)
    dx = np.where(kind == 1, sx * wobble, sx * np.where(kind == 2, W / np.hypot(W, H), 1.0))
    dy = np.where(kind == 0, sy * wobble, sy * np.where(kind == 2, H / np.hypot(W, H), 1.0))
    dz = np.where(i // 12 % 2, -1.0, 1.0) * rng.uniform(0.0004, 0.004, n)
    d = np.stack([dx, dy, dz], axis=1) * rng.uniform(0.5, 2.0, n)[:, None]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


# ---- cameras: (name, position, yaw, pitch, zoom) ----------------------------------------------------------------------------
# CameraController looks along (cos yaw cos pitch, sin pitch, sin yaw cos pitch).  The ray of a pixel is normalize(cam_dir) + sx *
# cam_right + sy * cam_up * H / W with sx, sy in -1 .. 1: a push whose cam_right and cam_up are 1 / zoom long sees a frame 2 / zoom
# wide at distance 1.
_ALONG = {(0, 1): (0.0, 0.0), (0, -1): (180.0, 0.0), (1, 1): (90.0, 86.0), (1, -1): (90.0, -86.0), (2, 1): (90.0, 0.0), (2, -1): (270.0, 0.0)}


def needle_cameras(dims):
    """Beyond the far (high) end looking back along the axis; inside, 96 voxels before the far cap, looking towards it; in the
    middle looking along the axis; beside the needle looking across its last voxels.  A needle is empty but for its caps and
    a few single voxels, so the views along it are narrow ones (zoom 10 and 150: the far cap, 96 and 2100 voxels away, fills a third and a fifth
    of the frame's width); the view from the side stands 14 voxels off and sees the last dozen voxels."""
    a = long_axis(dims)
    L = dims[a]
    u, v = [b for b in range(3) if b != a]
    mid = np.array(dims, np.float64) / 2 + 0.13

    def at(along, du=0.0):
        p = mid.copy(); p[a] = along; p[u] += du
        return tuple(float(t) for t in p)
    back, fwd = _ALONG[(a, -1)], _ALONG[(a, 1)]
    across = {0: (0.0, 0.0), 1: (90.0, 80.0), 2: (90.0, 0.0)}[u]
    return [("beyond the far end", at(L + 9.3), back[0] + 4.0, back[1] + 3.0, 1.0),
            ("inside near 4000", at(L - 96.4), fwd[0] + 0.3, fwd[1] + 0.2, 10.0),
            ("in the middle", at(L / 2 - 70.3), fwd[0] + 0.01, 89.99 if a == 1 else 0.01, 150.0),
            ("from the side", at(L - 4.7, du=-(dims[u] / 2 + 14.0)), across[0] + 2.0, across[1] + 1.0, 2.0)]


def slab_cameras(dims):
    """above the far corner looking down obliquely (towards +x, +y and into the slab); inside, eight voxels from the far corner,
    looking back along the slab's diagonal"""
    W, H, D = dims
    return [("above the far corner", (W - 70.3, H - 60.4, -25.6), 45.0, 35.0, 1.0),
            ("inside the far corner", (W - 9.4, H - 7.3, 1.6), 180.0, -float(np.degrees(np.arctan2(H, W))), 1.0)]


def push_of(vrt, dims, res, cam, frame=1):
    _, pos, yaw, pitch, zoom = cam
    push = vrt.make_push(vrt.CameraController(position=pos, yaw=yaw, pitch=pitch), dims, res, frame)
    for k in range(3):
        push.cam_right[k] = float(np.float32(push.cam_right[k]) / np.float32(zoom))
        push.cam_up[k] = float(np.float32(push.cam_up[k]) / np.float32(zoom))
    return push


def render_settings(vrt, res):
    """(name, settings): the reference's defaults (AO, shadow, bounces) at maxRaySteps 1024 -- the look-up loops and the AO pool; the
    same at 5000 -- the general march; primary rays only at 1024 -- the sky span, and the primary rays alone through the look-up
    loop.  The threshold runs are NOT among the paths of a dense scene here: the launch code sets df_thresh only while the
    longest axis is at most 1022 (vrt_api.hip, vrt_api_query.hip), and every dense scene of this file has one above it, so at a
    4096 axis and on the slabs the dense primary rays take the look-up loop without them.  Only the brick needles reach a
    threshold march, brick_march_thresh."""
    out = []
    for name, steps, primary in (("defaults, 1024", 1024, False), ("defaults, 5000", 5000, False), ("primary only, 1024", 1024, True)):
        st = vrt.VoxelRenderSettings.primary_only(res) if primary else vrt.VoxelRenderSettings(targetResolution=res)
        st.fsrSetttings.enable = False
        st.traceSettings.maxRaySteps = steps
        out.append((name, st))
    return out
