"""Shared by tests/test_render_rays_cpu.py and tests/test_gpu_render_rays.py: how ANY primary ray is checked against the oracle's
main() without changing the oracle, the two camera ray sets and the edge classes of the tests, and the scenes.

A push block with cam_right = cam_up = 0, jitter 0, cam_pos = origin, cam_dir = dir and screen_size = (W, H) gives every pixel of
the oracle's frame the same primary ray, and the noise coordinate depends on (px, py) only.  So ray i of a W x H frame is checked
as pixel (px, py) = (i % W, i // W) of a frame rendered under such a push: the test feeds (start, d') = oracle.primary_ray(push_i, px,
py) -- d' is the oracle's own renormalisation of dir (about a quarter of a panorama's unit directions change in the last bit, a
-0 component becomes +0) -- and compares every plane at that pixel with oracle.render(scene, push_i, params, rows=(py, py + 1))."""
import numpy as np

import raygen_reference as ref
from ray_query_common import edge_rays

W, H = 44, 28          # 1 232 rays: the last wave of the primary kernel holds 16, the last workgroup of the shading kernel is part filled
FRAME = 3
ORTHO = dict(pos=(16.3, 15.2, -10.0), cam_dir=(0.2, -0.1, 1.0), right=(1.0, 0.0, -0.2), up=(0.0, -1.0, 0.1), half_width=20.0)
PANORAMA_AT = (16.5, 30.5, 16.5)
GB_PLANES = ("color8", "depth", "motion", "mask8", "position", "normal8")
ALL_PLANES = GB_PLANES + ("color_f", "hit_id", "hit_voxel", "hit_mask")
EDGE = ("axis1", "axis2", "lattice_in")


def scene_a(vrt):
    """(volume, palette, sky, noise) of Scene A."""
    from helpers import metallic_palette
    vol = vrt.synthetic.floating_cubes(32, seed=1, count=40)
    return vol, metallic_palette(vrt), vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)


def ortho_rays(w=W, h=H, **over):
    return ref.camera_rays(ref.ORTHOGRAPHIC, w, h, **dict(ORTHO, **over))


def panorama_rays(w=W, h=H, at=PANORAMA_AT):
    return ref.camera_rays(ref.PANORAMA, w, h, pos=at)


def solid_origin_rays(rng, n, vol):
    """Rays whose origin lies inside a solid voxel: the march hits in iteration 0 with mask 0 -- rule A's zero normal, the general
    branch of the hit normal."""
    z, y, x = np.nonzero(vol)
    pick = rng.integers(0, len(x), n)
    o = np.stack([x[pick], y[pick], z[pick]], axis=1) + rng.uniform(0.1, 0.9, (n, 3))
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32)


def edge_class_rays(vol, per_class=256, solid=64, seed=77):
    """per_class rays of each class of EDGE and `solid` rays from inside solid voxels, one class after the other."""
    D, Hh, Ww = vol.shape
    rng = np.random.default_rng(seed)
    parts = [edge_rays(rng, per_class, (Ww, Hh, D), cls, vol) for cls in EDGE] + [solid_origin_rays(rng, solid, vol)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


MIXED_LABELS = ("orthographic", "panorama") + EDGE + ("solid_origin",)


def mixed_rays(vol, w=W, h=H):
    """(origins, dirs, labels) of one w x h frame: the two cameras' rays and the edge classes of edge_class_rays interleaved ray by
    ray (camera, camera, edge, camera, ...), each set subsampled evenly so that EVERY class lies inside the frame: a third of the
    frame each for the cameras, and the last third dealt in turn to axis1, axis2, lattice_in and the origins inside solid voxels
    (all 64 of those).  labels[i]: index into MIXED_LABELS of ray i's class."""
    n = w * h
    per_class, solid = 256, 64
    eo, ed = edge_class_rays(vol, per_class, solid)
    n_edge = n // 3
    n_cam = (n - n_edge + 1) // 2, (n - n_edge) // 2
    rest = n_edge - solid
    counts = [rest // 3 + (1 if k < rest % 3 else 0) for k in range(3)]
    assert max(counts) <= per_class
    picks, labs = [], []
    for k, c in enumerate(counts):
        picks.append(k * per_class + np.linspace(0, per_class - 1, c).round().astype(int)); labs.append(np.full(c, 2 + k))
    picks.append(3 * per_class + np.arange(solid)); labs.append(np.full(solid, 5))
    # within the edge share the classes take turns too
    order = np.argsort(np.concatenate([np.arange(len(q)) / len(q) for q in picks]), kind="stable")
    e_idx, e_lab = np.concatenate(picks)[order], np.concatenate(labs)[order]
    sets = []
    for k, (o, d) in enumerate((ortho_rays(w, h), panorama_rays(w, h))):
        idx = np.linspace(0, len(o) - 1, n_cam[k]).round().astype(int)
        sets.append((o[idx], d[idx], np.full(len(idx), k)))
    sets.append((eo[e_idx], ed[e_idx], e_lab))
    # camera, camera, edge in turn; whatever set runs out first simply stops taking turns
    slot = np.concatenate([(np.arange(len(q[0])) + (k + 1) / 4.0) / len(q[0]) for k, q in enumerate(sets)])
    order = np.argsort(slot, kind="stable")
    o = np.concatenate([q[0] for q in sets])[order]; d = np.concatenate([q[1] for q in sets])[order]
    labels = np.concatenate([q[2] for q in sets])[order]
    assert len(o) == n
    return np.ascontiguousarray(o, np.float32), np.ascontiguousarray(d, np.float32), labels


def pixel_push(oracle, dims, w, h, origin, direction, frame):
    p = oracle.Push()
    p.cam_pos[:] = [float(origin[0]), float(origin[1]), float(origin[2]), 1.0]
    p.cam_dir[:] = [float(direction[0]), float(direction[1]), float(direction[2]), 0.0]
    p.volume_bounds[:] = [int(dims[0]), int(dims[1]), int(dims[2])]
    p.frame = int(frame)
    p.screen_size[:] = [int(w), int(h)]
    return p


def oracle_frame(oracle, osn, params, w, h, origins, dirs, frame, planes=ALL_PLANES + ("rays_total",)):
    """(starts, dirs', planes): the rays to feed and the oracle's planes (h, w, ...) of the frame whose pixel (i % w, i // w) has
    the primary ray (origins[i], dirs[i]).  Fewer rays than w * h: the remaining pixels keep zeros and the rays returned are as
    many as were given."""
    n = len(origins)
    assert n <= w * h
    starts = np.zeros((n, 3), np.float32); dn = np.zeros((n, 3), np.float32)
    out = None
    for i in range(n):
        px, py = i % w, i // w
        push = pixel_push(oracle, osn.dims, w, h, origins[i], dirs[i], frame)
        starts[i], dn[i] = oracle.primary_ray(push, px, py)
        row = oracle.render(osn, push, params, planes=planes, rows=(py, py + 1))
        if out is None:
            out = {k: np.zeros_like(v) for k, v in row.items()}
        for k, v in row.items():
            out[k][py, px] = v[py, px]
    return starts, dn, out
