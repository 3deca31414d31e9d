"""Surface extraction without a GPU: the reference (tests/faces_reference.py) against its own properties and its plain-loop
restatement, the closed loop through the voxelizer's reference (faces -> quads -> triangles -> covered(SOLID) == occupancy), the
host build of csrc/vrt_faces.h against the reference on every box of the GPU tests' table, and the host-only entry points
(vrt_faces_mesh_host, vrt_faces_obj_host).  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import faces_common as fc
import faces_native as N
import faces_reference as R
import voxelize_reference as VR
from helpers import metallic_palette


def small(dims, seed, density=0.5):
    return fc._random(dims, seed, density)


@pytest.mark.parametrize("dims,lo,size", [((9, 7, 5), (0, 0, 0), (9, 7, 5)), ((9, 7, 5), (2, 1, 1), (6, 5, 3)), ((70, 3, 2), (1, 0, 0), (69, 3, 2)),
                                          ((3, 70, 2), (0, 2, 0), (3, 67, 2))])
def test_the_loops_give_the_arrays_records(dims, lo, size):
    vol = small(dims, 11)
    for runs, closed in fc.FLAGS:
        a, ca = R.faces(vol, lo, size, runs, closed)
        b, cb = R.faces_loops(vol, lo, size, runs, closed)
        assert (ca == cb).all() and a.shape == b.shape and (a == b).all(), (runs, closed)


def test_runs_expand_to_the_unit_list_and_both_are_in_order():
    vol = small((70, 9, 6), 5)
    lo, size = (1, 1, 0), (68, 7, 6)
    for closed in (False, True):
        unit, cu = R.faces(vol, lo, size, False, closed)
        runs, cr = R.faces(vol, lo, size, True, closed)
        assert (R.unpack(unit)[4] == 1).all() and int(R.unpack(runs)[4].max()) > 1 and runs.size < unit.size
        u, r = R.unit_faces(unit), R.unit_faces(runs)
        assert np.unique(u).size == u.size and (u == r).all()
        for rec, counts in ((unit, cu), (runs, cr)):
            d, key = R.order_keys(rec, size)
            assert (np.diff(d) >= 0).all() and (np.diff(key)[np.diff(d) == 0] > 0).all()
            assert (np.bincount(d, minlength=6) == counts).all()


def test_unit_faces_are_the_six_shifted_differences():
    vol = small((20, 9, 7), 8)
    solid = np.pad(vol != 0, 1)
    core = solid[1:-1, 1:-1, 1:-1]
    want = 0
    for axis in range(3):
        for step in (-1, 1):
            want += int((core & ~np.roll(solid, -step, axis)[1:-1, 1:-1, 1:-1]).sum())
    _, counts = R.faces(vol, (0, 0, 0), (20, 9, 7), False)
    assert int(counts.sum()) == want


def test_closed_differs_from_open_on_the_boundary_only():
    vol = small((24, 16, 12), 9, 0.7)
    lo, size = (3, 2, 1), (15, 9, 8)
    a = set(R.unit_faces(R.faces(vol, lo, size, False, False)[0]).tolist())
    b = set(R.unit_faces(R.faces(vol, lo, size, False, True)[0]).tolist())
    assert a <= b and len(b) > len(a)
    for key in b - a:
        x, y, z, d = key & 4095, (key >> 12) & 4095, (key >> 24) & 4095, key >> 44
        c = (x, y, z)[d >> 1]
        assert c == (size[d >> 1] - 1 if d & 1 else 0)


def test_quads_face_outwards_and_the_header_has_the_same_table():
    vol = small((8, 70, 4), 3)
    rec, _ = R.faces(vol, (0, 1, 0), (8, 68, 4), True)
    assert int(R.unpack(rec)[4].max()) > 2
    for r in rec[:: max(1, rec.size // 300)]:
        q = np.array(R.quad(r, (0, 0, 0)))
        d = int(R.unpack([r])[5][0])
        n = np.cross(q[1] - q[0], q[3] - q[0])
        want = np.zeros(3, np.int64)
        want[d >> 1] = 1 if d & 1 else -1
        assert (np.sign(n) == want).all() and (q[0] == q.min(axis=0)).all()
        assert (q[2] - q[0] == (q[1] - q[0]) + (q[3] - q[0])).all()
        assert N.quad(r) == [tuple(c) for c in q.tolist()]


def _round_trip(vol, lo, size, closed):
    rec, _ = R.faces(vol, lo, size, True, closed)
    v, q, _ = R.mesh(rec, lo)
    cover = VR.covered(v, R.triangles(q), VR.SOLID, (0, 0, 0), vol.shape[::-1])
    want = np.zeros(vol.shape, bool)
    sl = tuple(slice(lo[a], lo[a] + size[a]) for a in (2, 1, 0))
    want[sl] = vol[sl] != 0
    return cover, want


def test_round_trip_through_the_voxelizer_20x6x5():
    vol = small((20, 6, 5), 21)
    cover, want = _round_trip(vol, (0, 0, 0), (20, 6, 5), False)
    assert (cover == want).all()


def test_round_trip_with_runs_across_x_64():
    vol = small((70, 3, 2), 22, 0.8)
    assert int(R.unpack(R.faces(vol, (0, 0, 0), (70, 3, 2), True)[0])[0].max()) >= 64
    cover, want = _round_trip(vol, (0, 0, 0), (70, 3, 2), False)
    assert (cover == want).all()


def test_round_trip_of_a_closed_sub_box():
    vol = small((14, 8, 6), 23, 0.7)
    cover, want = _round_trip(vol, (3, 2, 1), (8, 5, 4), True)
    assert want.sum() > 50 and (cover == want).all()


@pytest.mark.parametrize("case", fc.CASES, ids=[c[0] for c in fc.CASES])
def test_the_header_on_the_host_gives_the_references_records(case):
    _, vol_name, lo, size = case
    for runs, closed in fc.FLAGS:
        want, wc = fc.expected(vol_name, lo, size, runs, closed)
        got, gc = N.faces(fc.volume(vol_name), lo, size, runs, closed)
        assert (gc == wc).all() and got.shape == want.shape and (got == want).all(), (case[0], runs, closed)


def test_what_the_table_is_there_for():
    """the bars split at 64 and 128 and nowhere else, alternating ids never merge, the checkerboard exposes everything, material
    around a box hides it, an empty box has nothing"""
    rec, _ = fc.expected("bars", (1, 1, 1), (140, 140, 5), True, False)
    bx, by, bz, vid, length, d = R.unpack(rec)
    for bar, along, dirs in ((9, bx, (2, 3, 4, 5)), (11, by, (0, 1))):
        for k in dirs:
            m = (vid == bar) & (d == k)
            assert along[m].tolist() == [3, 64, 128] and length[m].tolist() == [61, 64, 5], (bar, k)
    rec, counts = fc.expected("alternating", (0, 0, 0), (72, 8, 8), True, False)
    assert (R.unpack(rec)[4] == 1).all() and int(counts[4]) == 72 * 8 and int(counts[5]) == 72 * 8
    _, counts = fc.expected("checker", (0, 0, 0), (64, 8, 8), True, False)
    assert (counts == int((fc.volume("checker") != 0).sum())).all()
    assert fc.expected("solid", (5, 5, 5), (9, 10, 11), True, False)[1].sum() == 0
    rec, counts = fc.expected("solid", (5, 5, 5), (9, 10, 11), False, True)
    assert counts.tolist() == [110, 110, 99, 99, 90, 90]
    assert fc.expected("corner-brick", (9, 9, 9), (20, 20, 20), True, False)[0].size == 0


def test_the_stand_alone_program_under_the_sanitizers(tmp_path):
    lines = N.run_main_program(str(tmp_path / "faces_main_san"))
    assert len(lines) == 3 * 2 * 4
    for v, k, flags, *rest in lines:
        W, H, D = N.MAIN_DIMS[v]
        lo = (k, k, k)
        rec, counts = R.faces(N.main_volume(v), lo, (W - 2 * k, H - 2 * k, D - 2 * k), bool(flags & 1), bool(flags & 2))
        s = 0
        for r in rec.tolist():
            s = (s * 31 + r) & 0xFFFFFFFFFFFF
        assert rest[:6] == counts.tolist() and rest[6] == s, (v, k, flags)


# ---- host-only entry points ------------------------------------------------------------------------------------------------------

def test_mesh_host_equals_the_reference(vrt):
    vol = small((70, 9, 6), 31)
    lo = (1, 2, 0)
    for runs in (False, True):
        rec, _ = R.faces(vol, lo, (68, 6, 6), runs)
        v, q, ids = vrt.faces_mesh(rec, lo)
        ev, eq, eids = R.mesh(rec, lo)
        assert v.dtype == np.int32 and q.dtype == np.uint32 and ids.dtype == np.uint8
        assert v.shape == ev.shape and (v == ev).all() and (q == eq).all() and (ids == eids).all()
        assert (vrt.quads_to_triangles(q) == R.triangles(eq)).all()
    v, q, ids = vrt.faces_mesh(np.zeros(0, np.uint64), lo)
    assert v.shape == (0, 3) and q.shape == (0, 4) and ids.shape == (0,)


def test_the_bit_fields_at_their_edges(vrt):
    r = N.faces_host().faces_record_c(255, 255, 255, 255, 64, 5)
    assert r == 255 | 255 << 8 | 255 << 16 | 255 << 24 | 63 << 32 | 5 << 40 and N.faces_host().faces_record_valid_c(r)
    assert [int(t[0]) for t in R.unpack([r])] == [255, 255, 255, 255, 64, 5]
    v, q, ids = vrt.faces_mesh(np.array([r], np.uint64), (0, 0, 0))
    assert ids.tolist() == [255] and q.tolist() == [[0, 1, 2, 3]]
    assert v.tolist() == [[16 * c for c in p] for p in ((255, 255, 256), (319, 255, 256), (319, 256, 256), (255, 256, 256))]
    lib = vrt.lib()
    out = [C.c_void_p() for _ in range(3)]
    nv = C.c_uint64()
    lo = (C.c_int32 * 3)(0, 0, 0)
    for bad in (r | 1 << 38, r | 1 << 43, r | 1 << 63, (r & ~(7 << 40)) | 6 << 40, r & ~(255 << 24)):
        one = (C.c_uint64 * 1)(bad)
        assert lib.vrt_faces_mesh_host(one, 1, lo, C.byref(out[0]), C.byref(nv), C.byref(out[1]), C.byref(out[2])) == 1, hex(bad)
        assert not N.faces_host().faces_record_valid_c(bad)
    one = (C.c_uint64 * 1)(r)
    assert lib.vrt_faces_mesh_host(None, 1, lo, C.byref(out[0]), C.byref(nv), C.byref(out[1]), C.byref(out[2])) == 1
    assert lib.vrt_faces_mesh_host(one, 1, None, C.byref(out[0]), C.byref(nv), C.byref(out[1]), C.byref(out[2])) == 1
    assert lib.vrt_faces_mesh_host(one, 1, lo, None, C.byref(nv), C.byref(out[1]), C.byref(out[2])) == 1
    counts = (C.c_uint64 * 6)()
    size = (C.c_uint32 * 3)(1, 1, 1)
    assert lib.vrt_scene_list_faces(None, None, lo, size, 0, None, 0, counts) == 1 and b"vrt_scene_list_faces: NULL argument" in lib.vrt_last_error()
    assert lib.vrt_scene_save_obj_file(None, None, b"x.obj", 0) == 1 and b"vrt_scene_save_obj_file" in lib.vrt_last_error()


def test_the_encoded_obj_reads_back(vrt, tmp_path):
    vol = small((20, 9, 6), 41)
    vol[vol == 2] = 200
    pal = metallic_palette(vrt)
    lo = (3, 1, 2)
    rec, _ = R.faces(vol, (0, 0, 0), (20, 9, 6), True)
    obj, mtl = vrt.faces_obj_host(rec, lo, pal, "surface.mtl")
    assert obj.startswith(b"mtllib surface.mtl\nv ")
    (tmp_path / "s.obj").write_bytes(obj)
    v, t = vrt.read_obj(str(tmp_path / "s.obj"))
    ev, eq, eids = R.mesh(rec, lo)
    assert (v == ev).all()                                        # integer voxels in the file, x 16 by the reader
    by_id = np.argsort(eids, kind="stable")                       # groups in ascending id, the records' order within one
    assert (t == R.triangles(eq[by_id])).all()
    groups = [int(l.split(b"_")[1]) for l in obj.splitlines() if l.startswith(b"usemtl ")]
    assert groups == sorted(set(eids.tolist()))
    names = [int(l.split(b"_")[1]) for l in mtl.splitlines() if l.startswith(b"newmtl ")]
    assert names == groups
    kd = [tuple(float(w) for w in l.split()[1:]) for l in mtl.splitlines() if l.startswith(b"Kd ")]
    assert len(kd) == len(names)
    for vid, colour in zip(names, kd):
        assert (np.array(colour, np.float32) == np.asarray(pal, np.float32)[vid, :3]).all()      # %.9g round-trips a float32
