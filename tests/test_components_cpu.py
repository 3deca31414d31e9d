"""csrc/vrt_components.h on the host (tests/native/components_host.cpp): its sequential twin of the definition against the plain
breadth-first search of tests/components_reference.py on every scene the GPU tests use and on random volumes; known answers; the
argument rules; the record's layout against include/vrt.h's mirror in Python; the fuzz program under ASan and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_common as cc
import components_native as N
import components_reference as R


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_twin_equals_the_reference(name):
    vol = cc.volume(name)
    for match, conn, bounds in cc.CASES[name][1]:
        rc, rec, res, labels = N.components(vol, match, conn, bounds, cc.DTYPE)
        assert rc == 0
        cc.assert_same(rec, res, labels, cc.answer(name, match, conn, bounds), (name, match, conn, bounds))


def test_known_answers():
    def count(name, match, conn):
        return cc.answer(name, match, conn, None)[1]["components"]
    assert count("two_blobs", R.SOLID, 6) == 2 and count("two_blobs", R.SOLID, 26) == 2 and count("two_blobs", R.EMPTY, 6) == 1
    assert count("plus", R.SOLID, 6) == 1
    for kind in ("edge8", "edge12", "corner8", "corner12"):
        assert count(kind, R.SOLID, 6) == 2 and count(kind, R.SOLID, 26) == 1
    assert count("u", R.SOLID, 6) == 1 and count("serpentine", R.SOLID, 6) == 1 and count("ring", R.SOLID, 6) == 1
    assert count("late_root", R.SOLID, 6) == 3 and count("late_root", R.SOLID, 26) == 2
    rec = cc.answer("late_root", R.SOLID, 26, None)[0]
    assert tuple(rec[1]["root"]) == (7, 7, 7) and int(rec[1]["voxels"]) == 513 and tuple(rec[0]["root"]) == (1, 1, 1)
    assert count("touching_ids", R.SOLID, 6) == 2 and count("touching_ids", R.SAME, 6) == 3
    assert count("checkerboard", R.SOLID, 6) == 2048 and count("checkerboard", R.SOLID, 26) == 1 and count("checkerboard", R.EMPTY, 6) == 2048
    rec, res, _, _ = cc.answer("cavities", R.EMPTY, 6, None)
    assert res["components"] == 2 and int(rec[0]["faces"]) == 63 and res["largest"] == 0      # the leaking cavity is part of the outer air
    assert int(rec[1]["faces"]) == 0 and int(rec[1]["voxels"]) == 6 * 8 * 4 and tuple(rec[1]["lo"]) == (31, 7, 25)
    rec, res, labels, cl = cc.answer("off_grid", R.SOLID, 6, cc.OFF_GRID[1])
    assert cl == ((0, 0, 0), (16, 28, 12)) and labels.shape == (12, 28, 16)
    assert cc.answer("off_grid", R.SOLID, 6, cc.OFF_GRID[2])[1]["components"] > 0 and cc.answer("off_grid", R.SOLID, 6, cc.OFF_GRID[2])[3] == ((30, 30, 30), (10, 10, 10))


def test_random_small_volumes():
    rng = np.random.default_rng(7)
    for k in range(200):
        dims = tuple(int(v) for v in rng.integers(1, 20, 3))
        vol = ((rng.random((dims[2], dims[1], dims[0])) < rng.uniform(0.1, 0.9)) * rng.integers(1, 4, (dims[2], dims[1], dims[0]))).astype(np.uint8)
        match, conn = int(rng.integers(0, 3)), (6, 26)[int(rng.integers(0, 2))]
        bounds = None if k % 3 == 0 else (tuple(int(v) for v in rng.integers(-3, 6, 3)), tuple(int(v) for v in rng.integers(1, 24, 3)))
        records, result, labels, cl = R.components(vol, match, conn, bounds)
        rc, rec, res, lab = N.components(vol, match, conn, bounds, cc.DTYPE)
        assert rc == 0
        cc.assert_same(rec, res, lab, (R.records_array(records, cc.DTYPE), result, labels, cl), (k, dims, match, conn, bounds))


def test_filter_twin_equals_the_reference():
    rng = np.random.default_rng(9)
    some = 0
    for k in range(120):
        dims = tuple(int(v) for v in rng.integers(4, 18, 3))
        vol = ((rng.random((dims[2], dims[1], dims[0])) < rng.uniform(0.15, 0.7)) * rng.integers(1, 4, (dims[2], dims[1], dims[0]))).astype(np.uint8)
        match, conn = int(rng.integers(0, 3)), (6, 26)[int(rng.integers(0, 2))]
        kw = dict(bounds=None if k % 2 else ((-1, 1, 0), (12, 30, 9)), min_voxels=int(rng.integers(0, 3)), max_voxels=int(rng.integers(3, 40)),
                  faces_all=int(rng.integers(0, 64)) if k % 5 == 0 else 0, faces_none=int(rng.integers(0, 64)) if k % 3 == 0 else 0,
                  keep_largest=bool(k % 4 == 0), measure=bool(k % 7 == 0))
        vid = int(rng.integers(0, 5))
        exp_vol, exp = R.filter_components(vol, vid, match, conn, **kw)
        rc, got_vol, got = N.filter_components(vol, vid, match, conn, **kw)
        assert rc == 0 and got == exp and (got_vol == exp_vol).all(), (k, kw, got, exp)
        some += exp["changed"] != 0
    assert some > 30


def test_argument_rules():
    ok = (4, 4, 4)
    for match in (0, 1, 2):
        for conn in (6, 26):
            assert N.args_ok(match, conn, 0, ok) and R.args_ok(match, conn, 0, ok)
    assert N.args_ok(0, 6, 0, (1 << 30, 1, 1))
    for match, conn, flags, size in ((3, 6, 0, ok), (-1, 6, 0, ok), (0, 18, 0, ok), (0, 0, 0, ok), (0, 6, 1, ok), (0, 6, 0, (0, 4, 4)), (0, 6, 0, (4, 4, (1 << 30) + 1))):
        assert not N.args_ok(match, conn, flags, size) and not R.args_ok(match, conn, flags, size), (match, conn, flags, size)
    assert N.filter_ok(0, 0, 0, 0, 0) and N.filter_ok(1, 2 ** 64 - 1, 63, 63, 3)
    for a in ((2, 1, 0, 0, 0), (0, 1, 64, 0, 0), (0, 1, 0, 64, 0), (0, 1, 0, 0, 4)):
        assert not N.filter_ok(*a) and not R.filter_ok(*a), a
    assert N.sides_ok((512, 512, 512)) and not N.sides_ok((513, 1, 1)) and not N.sides_ok((1, 1, 513))
    for vid in (0, 1, 200, 255):
        for match in (0, 1, 2):
            assert N.key(match, vid) == R.key(match, vid)
    vol = np.zeros((2, 3, 600), np.uint8)
    assert N.components(vol, 0, 6, ((0, 0, 0), (513, 3, 2)), cc.DTYPE)[0] == 1
    assert N.components(vol, 2, 6, ((-50, 0, 0), (562, 3, 2)), cc.DTYPE)[2] == {"components": 1, "voxels": 512 * 6, "largest": 0}      # 512 after the clip


def test_forward_directions_are_half_of_the_neighbours():
    for conn in (6, 26):
        f = N.forward(conn)
        assert len(f) == conn // 2 and len(set(f)) == len(f)
        assert all((d[2], d[1], d[0]) > (0, 0, 0) for d in f)
        assert sorted(f + [(-d[0], -d[1], -d[2]) for d in f]) == sorted(R.OFFSETS[conn])


def test_record_layout(vrt):
    """csrc/vrt_components.h's CompRecord, include/vrt.h's vrt_component, _capi.Component and the numpy dtype are one layout"""
    size, off = N.record_layout()
    K = vrt._capi.Component
    assert size == C.sizeof(K) == cc.DTYPE.itemsize == vrt.VoxelScene.COMPONENT_DTYPE.itemsize == 56
    for name, o in off.items():
        assert getattr(K, name).offset == o == cc.DTYPE.fields[name][1] == vrt.VoxelScene.COMPONENT_DTYPE.fields[name][1], name
    assert cc.DTYPE == vrt.VoxelScene.COMPONENT_DTYPE
    hdr = open(os.path.join(N.ROOT, "include", "vrt.h")).read()
    body = re.search(r"typedef struct vrt_component \{(.*?)\} vrt_component;", hdr, re.S).group(1)
    assert re.findall(r"^\s*\w+\s+(\w+)(?:\[3\])?;", body, re.M) == ["root", "id", "voxels", "lo", "size", "faces", "reserved"]
    for name, val in (("SOLID", R.SOLID), ("SAME", R.SAME), ("EMPTY", R.EMPTY), ("FACES", 6), ("CORNERS", 26)):
        assert re.search(rf"#define VRT_COMP_{name}\s+{val}\b", hdr) and getattr(vrt._capi, "COMP_" + name) == val
    assert re.search(r"#define VRT_COMP_KEEP_LARGEST 1u", hdr) and re.search(r"#define VRT_COMP_MEASURE\s+2u", hdr)


def test_fuzz_program_under_asan_and_ubsan(tmp_path):
    """tests/native/components_fuzz.cpp, a program of its own, with -fsanitize=address,undefined and no recovery: the header's twin
    against a depth-first search, with bounds at the int32 edges; an overflow or an index out of range would end it"""
    src = os.path.join(N.ROOT, "tests", "native", "components_fuzz.cpp")
    exe = str(tmp_path / "components_fuzz_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, src])
    for seed in ("1", "2"):
        r = subprocess.run([exe, seed, "150"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
        m = re.match(r"(\d+) calls, (\d+) components", r.stdout)
        assert m and int(m.group(1)) == 150 and int(m.group(2)) >= 150, r.stdout      # not vacuous
