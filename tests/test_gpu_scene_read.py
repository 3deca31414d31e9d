"""Scene read-back on the GPU: vrt_scene_read_box and vrt_scene_list_box on dense and brick scenes against the numpy volume the
scene was built from (and edited with), vrt_scene_save_vox_mem against the host-only writer byte for byte and through the readers
and a render, the three kinds of stream behind a busy device, and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extents_common as ext
import scene_read_common as rc
import stream_common as sc
from helpers import camera_push
from ray_query_common import bricks_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "voxel-raytracing_amd", "host", "vrt_app")

SMALL = (37, 21, 19)
NINE_FIELDS = next(d for d, ok in ext.SLABS if ok)                  # the largest slice of the nine-field layout
EIGHT_FIELDS = next(d for d, ok in ext.SLABS if not ok)             # the first the eight-field layout takes
LIST_DIMS = (272, 16, 8)                                            # 34 x 2 x 1 bricks: room for a 256-wide box at an unaligned corner
LIST_LO = (5, 3, 1)


def _random_volume(dims, seed, p=0.3):
    W, H, D = dims
    rng = np.random.default_rng(seed)
    return ((rng.random((D, H, W)) < p) * rng.integers(1, 256, (D, H, W))).astype(np.uint8)


def _boxes(dims):
    """the whole volume, the eight corner voxels, a box on each face, an unaligned interior box: (lo, size)"""
    W, H, D = dims
    out = [((0, 0, 0), (W, H, D))]
    out += [(((W - 1) * (k & 1), (H - 1) * (k >> 1 & 1), (D - 1) * (k >> 2)), (1, 1, 1)) for k in range(8)]
    w, h, d = min(W, 7), min(H, 5), min(D, 3)
    mid = ((W - w) // 2, (H - h) // 2, (D - d) // 2)
    for a in range(3):
        for far in (0, 1):
            lo = list(mid)
            lo[a] = (dims[a] - (w, h, d)[a]) if far else 0
            out.append((tuple(lo), (w, h, d)))
    if min(dims) >= 3:
        out.append(((3 % W, 1, 1), (min(W - 3 % W - 1, 133), max(1, H - 3), max(1, D - 2))))
    return out


@pytest.mark.parametrize("dims", [SMALL, NINE_FIELDS, EIGHT_FIELDS], ids=["37x21x19", "nine fields", "eight fields"])
def test_read_box_dense(vrt, engine, dims):
    vol = _random_volume(dims, 11) if dims == SMALL else ext.slab_volume(dims)
    scene = vrt.VoxelScene.from_dense(engine, vol, rc.all_bytes_palette(vrt))
    try:
        for lo, size in _boxes(dims):
            got = scene.read(lo, size)
            assert got.shape == size[::-1]
            assert (got == rc.box_slice(vol, lo, size)).all(), (lo, size)
        whole, _ = scene.download()
        assert (whole == vol).all()                                     # vrt_scene_download as before
    finally:
        scene.destroy()


def test_read_box_past_the_32bit_field_limit(vrt, engine):
    """the 832^3 scene of tests/test_gpu_configs.py: 64-bit field offsets, no field 8.  Corners, far faces, an unaligned box and
    a listing, not the whole 576 MB"""
    N = 832
    vol = vrt.synthetic.sparse_bricks(N, 8, 0.004, seed=9)
    scene = vrt.VoxelScene.from_dense(engine, vol, rc.all_bytes_palette(vrt))
    try:
        boxes = [b for b in _boxes((N, N, N))[1:]] + [((N - 300, N - 40, N - 9), (300, 40, 9))]
        assert any(rc.box_slice(vol, lo, size).any() for lo, size in boxes)
        for lo, size in boxes:
            assert (scene.read(lo, size) == rc.box_slice(vol, lo, size)).all(), (lo, size)
        z, y, x = (int(t) for t in np.argwhere(vol[N // 2:])[0] + (N // 2, 0, 0))     # an occupied voxel in the upper half: above 2^31 bytes of a field
        size = (256, 100, 3)
        lo = tuple(min(max(0, c - s // 2), N - s) for c, s in zip((x, y, z), size))
        want = rc.records_of(vol, lo, size)
        assert want.size and (scene.voxels(lo, size) == want).all()
    finally:
        scene.destroy()


BRICK_DIMS = (40, 32, 24)                                               # 5 x 4 x 3 bricks


def _brick_volume():
    vol = _random_volume(BRICK_DIMS, 12, 0.2)
    vol[:, :, 16:24] = 0                                                # the bricks bx = 2: empty
    vol[8:16, 8:24, :] = 0                                              # and bz = 1, by = 1 .. 2
    return vol


def _brick_boxes():
    return [((0, 0, 0), BRICK_DIMS), ((16, 0, 0), (8, 32, 24)), ((17, 9, 9), (5, 13, 6)),       # whole; empty bricks only (twice)
            ((3, 5, 7), (30, 20, 11)), ((15, 7, 7), (10, 10, 10)), ((39, 31, 23), (1, 1, 1)), ((7, 0, 0), (2, 32, 24))]


def test_read_box_bricks(vrt, engine):
    vol = _brick_volume()
    grid, pool = bricks_of(vol)
    assert (grid == 0).any() and (grid != 0).any()
    scene = vrt.VoxelScene.from_bricks(engine, grid, pool, rc.all_bytes_palette(vrt))
    try:
        def agree(what):
            for lo, size in _brick_boxes():
                assert (scene.read(lo, size) == rc.box_slice(vol, lo, size)).all(), (what, lo, size)
                want = rc.records_of(vol, lo, size) if max(size) <= 256 else None
                if want is not None:
                    assert scene.count(lo, size) == want.size and (scene.voxels(lo, size) == want).all(), (what, lo, size)
        agree("as built")
        with pytest.raises(vrt.VrtError):
            scene.download()                                            # still refused: a brick scene has no dense volume
        scene.reserve_bricks(len(pool) + 3)
        agree("reserved")
        occ = lambda: (grid_of(vol) != 0)
        grid_of = lambda v: bricks_of(v)[0]
        before = occ()
        # one brick emptied (its slot is freed) ...
        victim = tuple(int(t) for t in np.argwhere(before)[0])          # (bz, by, bx)
        lo = (victim[2] * 8, victim[1] * 8, victim[0] * 8)
        scene.fill(lo, (8, 8, 8), 0); vol[lo[2]:lo[2] + 8, lo[1]:lo[1] + 8, lo[0]:lo[0] + 8] = 0
        assert int((before & ~occ()).sum()) == 1
        agree("a brick emptied")
        # ... a previously empty brick filled (it takes a slot, the freed one included), at an unaligned box inside it
        ids = _random_volume((5, 4, 3), 13, 0.9)
        scene.edit((18, 10, 9), ids); vol[9:12, 10:14, 18:23] = ids
        assert not before[1, 1, 2] and occ()[1, 1, 2]
        agree("an empty brick filled")
        # ... and an edit across brick boundaries that reaches into the empty column
        ids = _random_volume((12, 3, 2), 14, 0.8); ids[0, 0, 0] = ids[-1, -1, -1] = 7
        scene.edit((14, 3, 0), ids); vol[0:2, 3:6, 14:26] = ids
        agree("across bricks")
    finally:
        scene.destroy()


def _list_scene(vrt, engine, kind, vol):
    pal = rc.all_bytes_palette(vrt)
    if kind == "dense":
        return vrt.VoxelScene.from_dense(engine, vol, pal)
    grid, pool = bricks_of(vol)
    return vrt.VoxelScene.from_bricks(engine, grid, pool, pal)


@pytest.mark.parametrize("kind", ["dense", "brick"])
def test_list_box(vrt, engine, kind):
    lib = vrt.lib()
    for name, size, how in rc.LIST_BOXES + [("empty bricks only", (19, 8, 8), "empty bricks")]:
        vol = _random_volume(LIST_DIMS, 20 + len(name), 0.3)
        lo = LIST_LO
        if how == "empty bricks":
            vol[:, :, 64:96] = 0                                        # bricks bx = 8 .. 11 of every row: empty
            lo = (70, 8, 0)
        else:
            vol[lo[2]:lo[2] + size[2], lo[1]:lo[1] + size[1], lo[0]:lo[0] + size[0]] = rc.fill(size, how, seed=len(name))
        want = rc.records_of(vol, lo, size)
        scene = _list_scene(vrt, engine, kind, vol)
        try:
            assert scene.count(lo, size) == want.size, (name, kind)
            got = scene.voxels(lo, size)
            assert got.dtype == np.uint32 and got.size == want.size and (got == want).all(), (name, kind)
            if how in ("empty", "empty bricks"):
                assert want.size == 0
            if how == "solid":
                assert want.size == size[0] * size[1] * size[2]
            if want.size > 1:
                clo, csz = (C.c_int32 * 3)(*lo), (C.c_uint32 * 3)(*size)
                n = C.c_uint64(0)
                guard = np.full(want.size + 8, 0xDEADBEEF, np.uint32)
                # capacity = count - 1: nothing written, the count reported
                rc_ = lib.vrt_scene_list_box(engine.ctx, scene.handle, clo, csz, guard.ctypes.data_as(C.c_void_p), want.size - 1, C.byref(n))
                assert rc_ == 1 and n.value == want.size and (guard == 0xDEADBEEF).all(), (name, kind)
                # capacity = count: exact, nothing behind the buffer touched
                n = C.c_uint64(0)
                rc_ = lib.vrt_scene_list_box(engine.ctx, scene.handle, clo, csz, guard.ctypes.data_as(C.c_void_p), want.size, C.byref(n))
                assert rc_ == 0 and n.value == want.size and (guard[:want.size] == want).all() and (guard[want.size:] == 0xDEADBEEF).all(), (name, kind)
            if name == rc.LIST_BOXES[0][0]:
                with pytest.raises(vrt.VrtError) as ei:
                    scene.count((0, 0, 0), (257, 1, 1))
                assert ei.value.code == 1 and "256" in str(ei.value)
                assert (scene.read((0, 0, 0), (257, 1, 1)) == rc.box_slice(vol, (0, 0, 0), (257, 1, 1))).all()      # read_box has no such limit
                for bad_lo, bad_size in (((0, 0, 0), (0, 1, 1)), ((270, 0, 0), (3, 1, 1)), ((0, -1, 0), (1, 1, 1))):
                    with pytest.raises(vrt.VrtError) as ei:
                        scene.read(bad_lo, bad_size)
                    assert ei.value.code == 1
        finally:
            scene.destroy()


def _gbuffer(vrt, engine, scene, dims):
    st = vrt.VoxelRenderSettings(targetResolution=(96, 64))
    st.fsrSetttings.enable = False
    push = camera_push(vrt, dims, (96, 64), frame=3)
    g = vrt.GeometryStage(engine, st, scene).record(push)
    engine.synchronize()
    return g.numpy()


@pytest.mark.parametrize("kind", ["dense", "brick"])
def test_save(vrt, oracle, engine, kind):
    pal = rc.all_bytes_palette(vrt)
    if kind == "dense":
        dims = (300, 37, 258)
        vol = _random_volume(dims, 31, 0.004)
        vol[100:140, 5:30, 120:170] = _random_volume((50, 25, 40), 32, 0.5)        # something to look at
        scene = vrt.VoxelScene.from_dense(engine, vol, pal)
    else:
        dims = (520, 8, 16)                                             # 65 x 1 x 2 bricks: three tiles along x
        vol = _random_volume(dims, 33, 0.05)
        vol[:, :, 256:384] = 0
        grid, pool = bricks_of(vol)
        scene = vrt.VoxelScene.from_bricks(engine, grid, pool, pal)
        scene.reserve_bricks(len(pool) + 8)
        ids = _random_volume((20, 6, 9), 34, 0.7)
        scene.edit((250, 1, 3), ids); vol[3:12, 1:7, 250:270] = ids
        scene.fill((500, 0, 0), (20, 8, 8), 0); vol[0:8, 0:8, 500:520] = 0
        read = scene.read((0, 0, 0), dims)
        assert (read == vol).all()
        vol = read                                                      # the volume from read_box, itself checked above
    try:
        data = scene.to_vox_bytes()
        assert data == vrt.vox_encode_host(vol, pal)
        if oracle.refvox() is not None:
            r, rvox, rpal, _, dropped = oracle.refvox_flatten(data)
            assert r == 0 and dropped == 0 and rvox.shape == vol.shape and (rvox == vol).all() and rc.same_bits(rpal, pal)
        ovox, opal, _, _ = vrt.vox_flatten_host(data)
        assert ovox.shape == vol.shape and (ovox == vol).all() and rc.same_bits(opal, pal)
        again = vrt.VoxelScene.from_memory(engine, data)
        try:
            a, b = _gbuffer(vrt, engine, scene, dims), _gbuffer(vrt, engine, again, dims)
            assert any(np.unique(v).size > 1 for v in a.values())           # the frame shows something
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (kind, k)
        finally:
            again.destroy()
    finally:
        scene.destroy()


def test_save_to_a_file(vrt, engine, tmp_path):
    vol = _random_volume(SMALL, 41)
    pal = rc.all_bytes_palette(vrt)
    scene = vrt.VoxelScene.from_dense(engine, vol, pal)
    try:
        scene.save(tmp_path / "s.vox")
        assert (tmp_path / "s.vox").read_bytes() == vrt.vox_encode_host(vol, pal)
        with pytest.raises(RuntimeError):
            scene.save(tmp_path / "no such directory" / "s.vox")        # VRT_ERR_IO
    finally:
        scene.destroy()


@pytest.mark.parametrize("kind", sc.KINDS)
def test_streams_behind_a_busy_device(vrt, kind):
    """edit, read_box, list_box, edit, save_vox_mem on the HIP null stream, the context's own stream and a side stream of the
    caller, enqueued behind a stall of tests/stream_common.py's size with no synchronise by the caller: each output equals what
    the numpy volume says at that point of the sequence."""
    import torch
    dims = (40, 24, 32)
    vol = _random_volume(dims, 51, 0.2)
    pal = rc.all_bytes_palette(vrt)
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        engine = vrt.Engine(0, use_torch_stream=kind != "own")
        dev = engine.torch_device
        lib, cap = vrt.lib(), vrt._capi
        scene = vrt.VoxelScene.from_dense(engine, vol, pal)
        stall_t, stall_p = None, C.c_void_p()
        if kind == "own":
            cap.check(lib.vrt_device_alloc(engine.ctx, sc.STALL_BYTES, C.byref(stall_p)))
        else:
            stall_t = torch.zeros(sc.STALL_BYTES // 4, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for k in range(sc.STALL_PASSES):                                 # the stall
            if kind == "own":
                cap.check(lib.vrt_memset(engine.ctx, stall_p, k, sc.STALL_BYTES))
            else:
                stall_t.add_(1.0)
        ids1 = _random_volume((9, 7, 5), 52, 0.8)
        scene.edit((3, 2, 1), ids1)
        v1 = vol.copy(); v1[1:6, 2:9, 3:12] = ids1
        box = ((1, 0, 0), (30, 20, 17))
        read = scene.read(*box)
        listed = scene.voxels(*box)
        scene.fill((5, 5, 2), (20, 3, 2), 0)
        v2 = v1.copy(); v2[2:4, 5:8, 5:25] = 0
        saved = scene.to_vox_bytes()
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        assert (read == rc.box_slice(v1, *box)).all(), kind
        assert (listed == rc.records_of(v1, *box)).all() and listed.size == np.count_nonzero(rc.box_slice(v1, *box)), kind
        assert (v1 != vol).any() and (v2 != v1).any()
        assert saved == vrt.vox_encode_host(v2, pal), kind
        scene.destroy(); engine.destroy()


def test_cpp_host_save_and_read(vrt, engine, tmp_path):
    """vrt_app --fill --save-vox --read-box on a .vox fixture: VoxelScene::save writes the file the Python mirror returns for the
    same scene after the same fill, VoxelScene::read the same box."""
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    path = os.path.join(ROOT, "tests", "golden", "vox_multi.vox")
    scene = vrt.VoxelScene(engine, path)
    try:
        dims = (scene.width, scene.height, scene.depth)
        lo = tuple(min(2, d - 1) for d in dims)
        size = tuple(max(1, min(5, d - l)) for d, l in zip(dims, lo))
        box = ((0, 0, 0), tuple(min(d, 9) for d in dims))
        out, ids = tmp_path / "saved.vox", tmp_path / "box.u8"
        r = subprocess.run([APP, "--vox", path, "--fill", *map(str, lo), *map(str, size), "9", "--save-vox", str(out),
                            "--read-box", *map(str, box[0]), *map(str, box[1]), str(ids)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        before = scene.to_vox_bytes()
        scene.fill(lo, size, 9)
        want = scene.to_vox_bytes()
        assert want != before and out.read_bytes() == want
        assert ids.read_bytes() == scene.read(*box).tobytes()
    finally:
        scene.destroy()
