"""The .vox writer (csrc/vox_writer.cpp, via the host-only C-ABI entry vrt_vox_encode_host) and the definitions of the scene
read-back (csrc/vrt_scene_read.h), without a device: what the writer writes, the reference's own parser (oracle/_ref, where it is
present) and the product's reader flatten back to the input bit for bit; the palette's quantisation rule; the records of a box
against np.nonzero; the checks that precede device work."""
import ctypes as C

import numpy as np
import pytest

import scene_read_common as rc


@pytest.fixture(scope="module")
def palette(vrt):
    return rc.all_bytes_palette(vrt)


@pytest.fixture(scope="module")
def native():
    return rc.native()


def _both_readers(vrt, oracle, data):
    """[(name, voxels, palette)] of the readers at hand: the product's always, the reference's parser where oracle/_ref is"""
    vox, pal, _, dropped = vrt.vox_flatten_host(data)
    assert dropped == 0
    out = [("own reader", vox, pal)]
    if oracle.refvox() is not None:
        r, rvox, rpal, _, rdropped = oracle.refvox_flatten(data)
        assert r == 0 and rdropped == 0
        out.append(("reference parser", rvox, rpal))
    return out


@pytest.mark.parametrize("case", rc.ROUND_TRIP, ids=[c[0] for c in rc.ROUND_TRIP])
def test_round_trip(vrt, oracle, palette, case):
    name, dims, make = case
    vol = make(dims)
    assert vol.shape == dims[::-1]
    data = vrt.vox_encode_host(vol, palette)
    assert data[:4] == b"VOX " and int.from_bytes(data[16:20], "little") == len(data) - 20
    for who, vox, pal in _both_readers(vrt, oracle, data):
        assert vox.shape == vol.shape, (who, vox.shape)
        assert (vox == vol).all(), who
        assert rc.same_bits(pal, palette), who                  # every colour float and every metallic value, bit for bit


def test_palette_covers_the_cases(vrt, palette):
    table = rc.loader_table(vrt)
    for k in range(4):
        assert set(palette[:, k].view(np.uint32)) == set(table.view(np.uint32))        # all 256 byte values in every channel
    want = [np.float32(0), np.float32(1), np.float32(0.37), np.float32(1) / np.float32(3), np.nextafter(np.float32(1), np.float32(0))]
    assert all((palette[:, 4].view(np.uint32) == w.view(np.uint32)).any() for w in want)


def test_the_sparse_case_has_empty_tiles(native):
    name, dims, make = rc.ROUND_TRIP[6]
    vol = make(dims)
    lo, size = C.c_uint32(), C.c_uint32()
    spans = []
    for a in range(3):
        n = native.scene_read_tiles(dims[a], 0, C.byref(lo), C.byref(size))
        axis = []
        for t in range(n):
            native.scene_read_tiles(dims[a], t, C.byref(lo), C.byref(size))
            axis.append((lo.value, size.value))
        spans.append(axis)
    assert [len(s) for s in spans] == [2, 2, 2] and spans[0] == [(0, 256), (256, 44)] and spans[2] == [(0, 256), (256, 2)]
    empty = sum(not rc.box_slice(vol, (x[0], y[0], z[0]), (x[1], y[1], z[1])).any() for z in spans[2] for y in spans[1] for x in spans[0])
    assert empty == 5
    # 4096: sixteen tiles; 257: a second tile of width 1
    assert native.scene_read_tiles(4096, 15, C.byref(lo), C.byref(size)) == 16 and (lo.value, size.value) == (3840, 256)
    assert native.scene_read_tiles(257, 1, C.byref(lo), C.byref(size)) == 2 and (lo.value, size.value) == (256, 1)


def test_loaded_fixtures_round_trip(vrt, oracle):
    paths = rc.loadable_fixtures()
    assert len(paths) >= 5
    for p in paths:
        data = open(p, "rb").read()
        vol, pal, _, _ = vrt.vox_flatten_host(data)
        again = vrt.vox_encode_host(vol, pal)
        for who, vox, pal2 in _both_readers(vrt, oracle, again):
            assert vox.shape == vol.shape and (vox == vol).all(), (p, who)
            assert rc.same_bits(pal2, pal), (p, who)


def test_quantisation_rule(vrt):
    """A float that is no byte's goes to the nearest table entry, an exact midpoint to the lower byte -- read off the file's RGBA
    chunk and held against the Python restatement of the table."""
    table = rc.loader_table(vrt)
    rng = np.random.default_rng(9)
    vals = list(rng.random(200).astype(np.float32)) + [np.float32(-0.25), np.float32(1.5), np.float32(1e-30)]
    mids = []
    for c in (0, 1, 17, 128, 200, 254):
        m = (np.float64(table[c]) + np.float64(table[c + 1])) / 2
        if np.float64(np.float32(m)) == m:                      # the midpoint is a float32: a true tie
            mids.append((c, np.float32(m)))
        vals += [np.nextafter(np.float32(m), np.float32(0)), np.nextafter(np.float32(m), np.float32(2))]
    assert len(mids) >= 2
    vals += [m for _, m in mids]
    vals = np.array(vals, np.float32)
    assert not any((table.view(np.uint32) == v.view(np.uint32)).any() for v in vals[:200])
    pal = np.zeros((256, 5), np.float32)
    ids = 1 + np.arange(vals.size)
    assert ids.max() < 256
    pal[ids, 1] = vals                                          # the green channel of ids 1 ..
    data = vrt.vox_encode_host(np.ones((1, 1, 1), np.uint8), pal)
    at = data.index(b"RGBA") + 12
    rgba = np.frombuffer(data[at:at + 1024], np.uint8).reshape(256, 4)
    got = rgba[ids - 1, 1]                                      # entry i colours id i + 1
    want = np.array([rc.colour_byte(table, v) for v in vals])
    assert (got == want).all(), np.nonzero(got != want)
    for c, m in mids:
        assert rc.colour_byte(table, m) == c                    # ties to the lower byte
    # and the quantised palette is what both readers give back
    vox, back, _, _ = vrt.vox_flatten_host(data)
    assert rc.same_bits(back[ids, 1], table[want])


@pytest.mark.parametrize("box", rc.LIST_BOXES, ids=[b[0] for b in rc.LIST_BOXES])
def test_record_definition(native, box):
    name, size, how = box
    dims = (size[0] + 5, size[1] + 3, size[2] + 2)
    lo = (3, 2, 1)
    vol = rc.fill(dims, "random", seed=3)
    vol[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = rc.fill(size, how, seed=len(name))
    want = rc.records_of(vol, lo, size)
    got = rc.native_list(native, vol, lo, size)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint32
    assert got.size == want.size == int(np.count_nonzero(rc.box_slice(vol, lo, size))) and (got == want).all()
    if how == "empty":
        assert got.size == 0
    if how == "solid":
        assert got.size == size[0] * size[1] * size[2]
    # the order is the box index's
    s = (C.c_uint32 * 3)(*size)
    idx = [native.scene_read_index(int(r & 255), int(r >> 8 & 255), int(r >> 16 & 255), s) for r in got[:: max(1, got.size // 50)]]
    assert idx == sorted(idx)


def test_box_checks_precede_device_work(native):
    dims = (300, 40, 20)
    big = 0xFFFFFFFF
    for max_side in (0, rc.LIST_MAX_SIDE):
        assert rc.native_check(native, dims, (0, 0, 0), (1, 1, 1), max_side) == (rc.CHECK_OK, 1)
        assert rc.native_check(native, dims, (44, 0, 0), (256, 40, 20), max_side) == (rc.CHECK_OK, 256 * 40 * 20)
        for a in range(3):
            size = [1, 1, 1]; size[a] = 0
            assert rc.native_check(native, dims, (0, 0, 0), size, max_side)[0] == rc.CHECK_EMPTY
            lo = [0, 0, 0]; lo[a] = -1
            assert rc.native_check(native, dims, lo, (1, 1, 1), max_side)[0] == rc.CHECK_OUTSIDE
            lo[a] = dims[a]
            assert rc.native_check(native, dims, lo, (1, 1, 1), max_side)[0] == rc.CHECK_OUTSIDE
            lo[a] = dims[a] - 1; size = [1, 1, 1]; size[a] = 2
            assert rc.native_check(native, dims, lo, size, max_side)[0] == rc.CHECK_OUTSIDE
        assert rc.native_check(native, dims, (0, 0, 0), (big, big, big), max_side)[0] == rc.CHECK_OVERFLOW     # 2^96 bytes
        assert rc.native_check(native, dims, (0, 0, 0), (big, big, 1), max_side)[0] != rc.CHECK_OVERFLOW       # below 2^64
    assert rc.native_check(native, dims, (0, 0, 0), (257, 1, 1), rc.LIST_MAX_SIDE)[0] == rc.CHECK_SIDE
    assert rc.native_check(native, dims, (0, 0, 0), (257, 1, 1), 0) == (rc.CHECK_OK, 257)
    assert rc.native_check(native, dims, (0, 0, 0), (1, 257, 1), rc.LIST_MAX_SIDE)[0] == rc.CHECK_SIDE
    assert rc.native_list(native, np.zeros((20, 40, 300), np.uint8), (0, 0, 0), (257, 1, 1)) == -1 - rc.CHECK_SIDE


def test_null_arguments(vrt):
    lib = vrt.lib()
    lo, size = (C.c_int32 * 3)(0, 0, 0), (C.c_uint32 * 3)(1, 1, 1)
    ids, recs, n64 = (C.c_uint8 * 1)(), (C.c_uint32 * 1)(), C.c_uint64()
    buf, n = C.c_void_p(), C.c_size_t()
    INVALID = 1
    assert lib.vrt_scene_read_box(None, None, lo, size, ids) == INVALID and b"vrt_scene_read_box: NULL argument" in lib.vrt_last_error()
    assert lib.vrt_scene_list_box(None, None, lo, size, recs, 1, C.byref(n64)) == INVALID and b"vrt_scene_list_box: NULL argument" in lib.vrt_last_error()
    assert lib.vrt_scene_save_vox_mem(None, None, C.byref(buf), C.byref(n)) == INVALID and b"vrt_scene_save_vox_mem" in lib.vrt_last_error()
    assert lib.vrt_scene_save_vox_file(None, None, b"x.vox") == INVALID and b"vrt_scene_save_vox_file" in lib.vrt_last_error()
    pal = vrt.host.materials_from_numpy(np.zeros((256, 5), np.float32))
    vox = (C.c_uint8 * 1)(1)
    dims = (C.c_uint32 * 3)(1, 1, 1)
    assert lib.vrt_vox_encode_host(None, dims, pal, C.byref(buf), C.byref(n)) == INVALID
    assert lib.vrt_vox_encode_host(vox, None, pal, C.byref(buf), C.byref(n)) == INVALID
    assert lib.vrt_vox_encode_host(vox, dims, None, C.byref(buf), C.byref(n)) == INVALID
    assert lib.vrt_vox_encode_host(vox, dims, pal, None, C.byref(n)) == INVALID
    assert lib.vrt_vox_encode_host(vox, dims, pal, C.byref(buf), None) == INVALID
    for bad in ((0, 1, 1), (1, 4097, 1)):
        assert lib.vrt_vox_encode_host(vox, (C.c_uint32 * 3)(*bad), pal, C.byref(buf), C.byref(n)) == INVALID
    assert lib.vrt_vox_encode_host(vox, dims, pal, C.byref(buf), C.byref(n)) == 0 and n.value > 1024
    lib.vrt_host_free(buf)


def test_a_file_is_a_function_of_the_content(vrt, palette):
    name, dims, make = rc.ROUND_TRIP[2]
    assert vrt.vox_encode_host(make(dims), palette) == vrt.vox_encode_host(make(dims).copy(), palette.copy())
