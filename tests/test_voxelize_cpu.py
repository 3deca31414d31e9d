"""The definition of vrt_scene_voxelize on the CPU: the analytic cases of the rules (tests/voxelize_reference.py, Python integers),
csrc/vrt_voxelize.h compiled for the host and held to that reference (tests/native/voxelize_host.cpp), the conservative rule
against polygon clipping in exact fractions, and the range-edge cases in a stand-alone program under the sanitizers."""
import numpy as np
import pytest

import voxelize_common as vc
import voxelize_native as N
import voxelize_reference as R


def solid_count(mesh, lo=(-2, -2, -2), size=(14, 14, 14)):
    return int(R.covered(mesh[0], mesh[1], R.SOLID, lo, size).sum())


def test_aligned_boxes_give_exactly_the_box():
    assert solid_count(vc.box_mesh((0, 0, 0), (64, 80, 96))) == 4 * 5 * 6
    c = R.covered(*vc.box_mesh((16, 32, 48), (48, 64, 64)), R.SOLID, (0, 0, 0), (6, 6, 6))
    exp = np.zeros((6, 6, 6), bool)
    exp[3:4, 2:4, 1:3] = True
    assert (c == exp).all()


def test_boxes_through_centres_give_the_half_open_count():
    mesh = vc.box_mesh((40, 40, 40), (104, 104, 104))                        # faces through the centres 40 and 104
    c = R.covered(mesh[0], mesh[1], R.SOLID, (0, 0, 0), (8, 8, 8))
    assert int(c.sum()) == 64
    zs, ys, xs = np.nonzero(c)
    assert len({int(xs.max()) - int(xs.min()), int(ys.max()) - int(ys.min()), int(zs.max()) - int(zs.min())}) == 1     # a 4 x 4 x 4 block


def _variants(mesh, rng):
    v, t = mesh
    yield "reversed order", (v, t[::-1].copy())
    yield "rotated vertices", (v, np.roll(t, 1, axis=1))
    yield "flipped winding", (v, t[:, ::-1].copy())
    yield "shuffled", (v, t[rng.permutation(len(t))])
    # the first triangle split along its edge v0 -> v1 at an integer point
    a, b, c = (v[int(i)].astype(np.int64) for i in t[0])
    m = a + (b - a) // 3 if ((b - a) % 3 == 0).all() else a + (b - a) // 2
    if ((m - a) * 2 == (b - a)).all() or ((m - a) * 3 == (b - a)).all():
        v2 = np.concatenate([v, m.reshape(1, 3).astype(np.int32)])
        k = np.uint32(len(v))
        t2 = np.concatenate([np.asarray([(t[0][0], k, t[0][2]), (k, t[0][1], t[0][2])], np.uint32), t[1:]])
        yield "split", (v2, t2)


def test_solid_does_not_depend_on_order_rotation_winding_or_splits():
    rng = np.random.default_rng(3)
    meshes = [vc.box_mesh((40, 40, 40), (104, 136, 72)), vc.tetra_mesh(((8, 8, 8), (8 + 192, 8, 8), (8, 8 + 192, 8), (8, 8, 8 + 192))),
              vc.tetra_mesh(((10, 22, 30), (170, 60, 44), (90, 190, 20), (100, 80, 180)))]
    seen = 0
    for mesh in meshes:
        base = R.covered(mesh[0], mesh[1], R.SOLID, (-1, -1, -1), (14, 14, 14))
        assert base.any()
        for name, m in _variants(mesh, rng):
            assert (R.covered(m[0], m[1], R.SOLID, (-1, -1, -1), (14, 14, 14)) == base).all(), name
            seen += name == "split"
    assert seen >= 2


def test_tetrahedra_agree_with_a_float_inside_test():
    rng = np.random.default_rng(11)
    checked = 0
    for _ in range(12):
        p = rng.integers(0, 200, (4, 3))
        vol6 = float(np.linalg.det((p[1:] - p[0]).astype(np.float64)))
        if abs(vol6) < 2e5:
            continue
        c = R.covered(*vc.tetra_mesh(p), R.SOLID, (0, 0, 0), (13, 13, 13))
        A = np.concatenate([p.T.astype(np.float64), np.ones((1, 4))])
        for z in range(13):
            for y in range(13):
                for x in range(13):
                    w = np.linalg.solve(A, np.asarray([16 * x + 8, 16 * y + 8, 16 * z + 8, 1.0]))       # barycentric coordinates
                    if np.abs(w).min() > 1e-6:                                # away from the surface
                        assert bool(c[z, y, x]) == bool((w > 0).all()), (p, x, y, z, w)
                        checked += 1
    assert checked > 10000


def test_degenerate_triangles_and_a_triangle_in_a_voxel_face():
    seg = ((8, 8, 8), (72, 40, 8), (72, 40, 8))
    pt = ((24, 24, 24),) * 3
    corner = ((32, 32, 32),) * 3
    c = R.meets_grid(seg, (-1, -1, -1), (6, 4, 2))
    assert c.any() and c.sum() < 16 and R.meets(seg, 0, 0, 0) and R.meets(seg, 4, 2, 0) and not R.meets(seg, 4, 0, 0)
    assert int(R.meets_grid(pt, (0, 0, 0), (3, 3, 3)).sum()) == 1 and R.meets(pt, 1, 1, 1)
    assert int(R.meets_grid(corner, (0, 0, 0), (3, 3, 3)).sum()) == 8          # a point on a voxel corner touches the eight around it
    face = ((16, 3, 3), (16, 13, 4), (16, 6, 12))                              # inside the face x = 16 of voxels (0,0,0) and (1,0,0)
    got = R.meets_grid(face, (-1, -1, -1), (3, 2, 2))
    assert int(got.sum()) == 2 and R.meets(face, 0, 0, 0) and R.meets(face, 1, 0, 0)
    for tri in (seg, pt, corner):
        assert not R.flips_grid(tri, (-1, -1, -1), (6, 4, 2)).any()          # no area: n_x == 0, flips nothing
    assert R.flips(face, 0, 0, 0) and not R.flips(face, 1, 0, 0)             # (the face has n_x != 0: the centre at x = 8 lies before it)
    for tri in (seg, pt, corner, face):
        for x in range(-1, 7):
            for y in range(-1, 4):
                assert N.meets(tri, x, y, 0) == R.meets(tri, x, y, 0) == vc.clip_meets(tri, x, y, 0)


def test_surface_is_what_polygon_clipping_says():
    rng = np.random.default_rng(5)
    n = 0
    for k in range(40):
        v, t = vc.random_mesh(rng, 1, -20, 110) if k % 4 else tri_on_grid(rng)
        tri = [tuple(int(c) for c in v[int(i)]) for i in t[0]]
        got = R.meets_grid(tri, (-2, -2, -2), (7, 7, 7))
        for z in range(-2, 8):
            for y in range(-2, 8):
                for x in range(-2, 8):
                    assert bool(got[z + 2, y + 2, x + 2]) == vc.clip_meets(tri, x, y, z), (tri, x, y, z)
                    n += bool(got[z + 2, y + 2, x + 2])
    assert n > 500


def tri_on_grid(rng):
    """vertices on voxel corners, edges and faces: the closed comparisons decide"""
    v = (rng.integers(-1, 7, (3, 3)) * 16 + rng.choice([0, 0, 8], (3, 3))).astype(np.int32)
    return v, np.asarray([(0, 1, 2)], np.uint32)


def test_scalar_and_array_forms_of_the_reference_agree():
    rng = np.random.default_rng(6)
    for _ in range(30):
        v, t = vc.random_mesh(rng, 1, -30, 90)
        g = R.meets_grid(v, (-2, -2, -2), (5, 5, 5))
        for z in range(-2, 6):
            for y in range(-2, 6):
                for x in range(-2, 6):
                    assert bool(g[z + 2, y + 2, x + 2]) == R.meets(v, x, y, z)


def test_a_solid_in_two_halves_equals_the_solid_in_one_piece():
    mesh = vc.merge(vc.torus_mesh((12.0, 11.5, 6.2), 7.0, 3.1, 10, 6), vc.tetra_mesh(((-90, 20, 30), (500, 60, 44), (90, 390, 20), (100, 80, 280))))
    lo, size = (0, 0, 0), (24, 24, 14)
    for fill in (R.SOLID, R.SOLID | R.SURFACE):
        whole = R.covered(mesh[0], mesh[1], fill, lo, size)
        assert whole.any()
        for axis, cut in ((0, 9), (0, 23), (1, 11), (2, 5)):
            la, sa, lb, sb = list(lo), list(size), list(lo), list(size)
            sa[axis] = cut
            lb[axis], sb[axis] = cut, size[axis] - cut
            a, b = R.covered(mesh[0], mesh[1], fill, la, sa), R.covered(mesh[0], mesh[1], fill, lb, sb)
            assert (np.concatenate([a, b], axis=2 - axis) == whole).all(), (fill, axis, cut)
        rc, got, _ = N.cover(mesh[0], mesh[1], fill, (0, 0, 0), (9, 24, 14))      # the header's whole-row flips: the mesh goes on beyond x = 9
        assert rc == 0 and (got == whole[:, :, :9]).all()


def test_header_against_the_reference_on_random_meshes():
    rng = np.random.default_rng(1)
    total = 0
    for k in range(60):
        v, t = vc.random_mesh(rng, int(rng.integers(1, 9)), -60, 420)
        if k % 3 == 0:
            v = (v // 8 * 8).astype(np.int32)                                # centres and faces get hit exactly
        for fill in (1, 2, 3):
            lo = tuple(int(x) for x in rng.integers(-3, 8, 3))
            size = tuple(int(x) for x in rng.integers(1, 22, 3))
            exp = R.covered(v, t, fill, lo, size)
            rc, got, _ = N.cover(v, t, fill, lo, size)
            assert rc == 0 and (got == exp).all(), (k, fill, lo, size, int(exp.sum()), int(got.sum()))
            total += int(exp.sum())
    assert total > 20000
    for name, mesh in (("torus", vc.torus_mesh((24.0, 24.0, 12.0), 14.0, 5.0)), ("sphere", vc.sphere_mesh((20.3, 22.1, 11.7), 9.4))):
        exp = R.covered(mesh[0], mesh[1], 3, (0, 0, 0), (70, 48, 24))       # a row of more than one mask word
        rc, got, _ = N.cover(mesh[0], mesh[1], 3, (0, 0, 0), (70, 48, 24))
        assert rc == 0 and (got == exp).all(), name


def test_header_pieces():
    for m, M in ((0, 0), (16, 16), (-1, 1), (-16, -16), (-17, 15), (5, 40), (-65536, 131072), (131072, 131072), (-65536, -65536)):
        assert N.axis_span(m, M) == R.voxel_span(m, M), (m, M)
    rng = np.random.default_rng(8)
    for _ in range(300):
        tri = rng.integers(-200, 700, (3, 3))
        if rng.random() < 0.3:
            tri = tri // 16 * 16 + 8                                         # crossings exactly at centres: the strict comparison decides
        y, z, x0, size_x = (int(t) for t in (rng.integers(-2, 40), rng.integers(-2, 40), rng.integers(-5, 30), rng.integers(1, 70)))
        col = R.flips_grid(tri, (x0, y, z), (x0 + size_x - 1, y, z))[0, 0]
        n = R.cross(R.sub(tri[1], tri[0]), R.sub(tri[2], tri[0]))
        if int(n[0]) != 0 and col.any():
            k = N.cross_count(tri, x0, size_x, y, z)
            assert col[:k].all() and not col[k:].any(), (tri, x0, size_x, y, z, k)
        for x in range(x0, x0 + min(size_x, 6)):
            assert N.flips(tri, x, y, z) == bool(col[x - x0])


def test_refusals_of_the_host_restatement():
    v, t = vc.box_mesh((0, 0, 0), (64, 64, 64))
    assert N.cover(v, t, 1, (0, 0, 0), (4, 4, 4))[0] == 0
    bad = v.copy(); bad[3, 1] = R.COORD_MAX + 1
    low = v.copy(); low[0, 0] = R.COORD_MIN - 1
    t_bad = t.copy(); t_bad[5, 2] = 8
    assert N.cover(bad, t, 1, (0, 0, 0), (4, 4, 4))[0] == 1 and N.cover(low, t, 1, (0, 0, 0), (4, 4, 4))[0] == 1
    assert N.cover(v, t_bad, 1, (0, 0, 0), (4, 4, 4))[0] == 1
    assert N.cover(v, t, 0, (0, 0, 0), (4, 4, 4))[0] == 1 and N.cover(v, t, 4, (0, 0, 0), (4, 4, 4))[0] == 1
    assert N.cover(v, t, 1, (0, 0, 0), (513, 4, 4))[0] == 1 and N.cover(v, t, 1, (0, 0, 0), (0, 4, 4))[0] == 1


def test_overflow_bounds_at_the_range_edges(tmp_path):
    """vertices at -65536 and 131072 against voxels at both ends of a 4096-voxel axis: Python integers say what is covered, the
    header agrees, and the stand-alone program built with -fsanitize=signed-integer-overflow,address runs the same cases clean"""
    size = (32, 32, 32)
    lines = {(k, c, f): (n, s) for k, c, f, n, s in N.run_edge_program(str(tmp_path / "voxelize_main_san"))}
    assert len(lines) == len(N.EDGE_CASES) * 2 * 3
    tri = np.asarray([(0, 1, 2)], np.uint32)
    biggest = 0
    for k, case in enumerate(N.EDGE_CASES):
        v = np.asarray(case, np.int64).reshape(3, 3)
        n = R.cross(R.sub(R.ints(v)[1], R.ints(v)[0]), R.sub(R.ints(v)[2], R.ints(v)[0]))
        biggest = max(biggest, max(abs(t) for t in n))
        for c, lo in enumerate(N.EDGE_CORNERS):
            for fill in (1, 2, 3):
                exp = R.covered(v, tri, fill, lo, size)
                idx = np.flatnonzero(exp.reshape(-1)).astype(object)
                assert lines[(k, c, fill)] == (int(exp.sum()), int((idx * idx).sum())), (k, c, fill)
                rc, got, _ = N.cover(v, tri, fill, lo, size)
                assert rc == 0 and (got == exp).all()
    assert biggest == 196608 ** 2 < 2 ** 37                                  # the largest component a normal can have (twice the area of half the range's square)


def test_mesh_units_and_the_obj_reader(vrt, tmp_path):
    pkg = vrt
    f = np.asarray([(0.03125, 0.09375, -0.03125), (1.0, 2.5, 8191.96875), (-4096.0, 0.15625, 0.21875)], np.float32)
    u = pkg.mesh_units(f)
    assert u.dtype == np.int32 and u.tolist() == [[0, 2, 0], [16, 40, 131072], [-65536, 2, 4]]        # ties go to even: 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, 3.5 -> 4
    assert (u == vc.units(f)).all()
    assert pkg.mesh_voxel_bounds(u) == R.mesh_bounds(u)
    verts = [(0.5, 0.5, 0.5), (4.5, 0.5, 0.5), (4.5, 3.5, 0.5), (0.5, 3.5, 0.5), (2.0, 2.0, 5.0)]
    faces = [(0, 3, 2, 1), (0, 1, 4), (1, 2, 4), (2, 3, 4), (3, 0, 4)]
    read = []
    for k, (rel, sl) in enumerate(((False, False), (True, True))):
        path = str(tmp_path / f"pyramid{k}.obj")
        vc.write_obj(path, verts, faces, rel, sl)
        read.append(pkg.read_obj(path))
    assert read[0][1].tolist() == [[0, 3, 2], [0, 2, 1], [0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4]]
    assert (read[0][0] == pkg.mesh_units(verts)).all() and all((a == b).all() for a, b in zip(read[0], read[1]))
    assert solid_count(read[0], (0, 0, 0), (6, 6, 6)) > 10
