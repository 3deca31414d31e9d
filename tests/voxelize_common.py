"""What the tests of vrt_scene_voxelize share: small meshes (integers, sixteenths of a voxel) and a polygon-clipping check of
the conservative rule that shares nothing with the 13-axis test."""
from fractions import Fraction

import numpy as np

U = 16


def box_mesh(lo, hi, flip=False):
    """the closed box lo..hi (mesh units), 12 triangles, outward winding (inward with flip)"""
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    v = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    quads = [(0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3)]
    t = []
    for a, b, c, d in quads:
        t += [(a, b, c), (a, c, d)]
    t = np.asarray(t, np.uint32)
    return np.asarray(v, np.int32), t[:, ::-1].copy() if flip else t


def tetra_mesh(p):
    """four points -> the closed tetrahedron"""
    return np.asarray(p, np.int32), np.asarray([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.uint32)


def merge(*meshes):
    vs, ts, base = [], [], 0
    for v, t in meshes:
        vs.append(np.asarray(v, np.int32))
        ts.append(np.asarray(t, np.uint32) + np.uint32(base))
        base += len(v)
    return np.concatenate(vs), np.concatenate(ts)


def units(v):
    """float voxels -> mesh units by the library's rule, restated: rint(float32(v) * 16)"""
    return np.rint(np.asarray(v, np.float32) * np.float32(16)).astype(np.int32)


def torus_mesh(centre, R, r, nu=12, nv=8):
    """a closed torus around the z axis through `centre` (voxels)"""
    v, t = [], []
    for i in range(nu):
        a = 2 * np.pi * i / nu
        for j in range(nv):
            b = 2 * np.pi * j / nv
            v.append((centre[0] + (R + r * np.cos(b)) * np.cos(a), centre[1] + (R + r * np.cos(b)) * np.sin(a), centre[2] + r * np.sin(b)))
    for i in range(nu):
        for j in range(nv):
            p, q, s, w = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            t += [(p, q, s), (p, s, w)]
    return units(v), np.asarray(t, np.uint32)


def sphere_mesh(centre, r, nu=12, nv=8):
    """a closed UV-sphere (voxels)"""
    v = [(centre[0], centre[1], centre[2] - r)]
    for j in range(1, nv):
        b = np.pi * j / nv
        for i in range(nu):
            a = 2 * np.pi * i / nu
            v.append((centre[0] + r * np.sin(b) * np.cos(a), centre[1] + r * np.sin(b) * np.sin(a), centre[2] - r * np.cos(b)))
    v.append((centre[0], centre[1], centre[2] + r))
    top, t = len(v) - 1, []
    ring = lambda j, i: 1 + (j - 1) * nu + i % nu
    for i in range(nu):
        t.append((0, ring(1, i + 1), ring(1, i)))
        t.append((top, ring(nv - 1, i), ring(nv - 1, i + 1)))
        for j in range(1, nv - 1):
            t += [(ring(j, i), ring(j, i + 1), ring(j + 1, i + 1)), (ring(j, i), ring(j + 1, i + 1), ring(j + 1, i))]
    return units(v), np.asarray(t, np.uint32)


def tiny_triangles(n, dims, seed):
    """n triangles, each well inside the size of a voxel, spread over the volume (some hang over its faces)"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, [U * d for d in dims], (n, 1, 3))
    v = (c + rng.integers(-5, 6, (n, 3, 3))).astype(np.int32).reshape(-1, 3)
    return v, np.arange(3 * n, dtype=np.uint32).reshape(-1, 3)


def random_mesh(rng, nt, lo, hi):
    """nt unrelated triangles with vertices in lo..hi (mesh units), a few of them degenerate"""
    v = rng.integers(lo, hi + 1, (3 * nt, 3)).astype(np.int32)
    for k in range(0, nt, 5):
        v[3 * k + 2] = v[3 * k + 1]                                  # a segment
    if nt > 3:
        v[9:12] = v[9]                                               # a point
    return v, np.arange(3 * nt, dtype=np.uint32).reshape(-1, 3)


def write_obj(path, verts_vox, faces, relative=False, slashes=False):
    """faces: lists of 0-based indices (polygons allowed)"""
    with open(path, "w") as f:
        f.write("# generated\n")
        for p in verts_vox:
            f.write("v %r %r %r\n" % (float(p[0]), float(p[1]), float(p[2])))
        for face in faces:
            idx = [(i - len(verts_vox)) if relative else i + 1 for i in face]
            f.write("f " + " ".join(("%d/%d/%d" % (i, 1, 1)) if slashes else str(i) for i in idx) + "\n")


# ---- the conservative rule by clipping: the triangle cut by the cube's six closed half-spaces is not empty -------------------------
def clip_meets(tri, x, y, z):
    poly = [tuple(Fraction(int(c)) for c in p) for p in tri]
    lo = (U * x, U * y, U * z)
    for a in range(3):
        for sign, bound in ((1, lo[a] + U), (-1, -lo[a])):            # sign * p[a] <= bound
            out = []
            for i, p in enumerate(poly):
                q = poly[(i + 1) % len(poly)]
                dp, dq = bound - sign * p[a], bound - sign * q[a]
                if dp >= 0:
                    out.append(p)
                if (dp > 0 and dq < 0) or (dp < 0 and dq > 0):
                    w = dp / (dp - dq)
                    out.append(tuple(p[k] + w * (q[k] - p[k]) for k in range(3)))
            poly = out
            if not poly:
                return False
    return True
