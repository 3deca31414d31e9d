"""vrt_scene_stamp on the GPU: dense and brick scenes in all four pairings, the 48 orientations of an asymmetric 5x3x2 source,
VRT_STAMP_SKIP_EMPTY, clipping at both ends, overlapping stamps of a scene onto itself, a source of three segments.  The checks
are test_gpu_brush.py's: the result and the whole volume against tests/brush_reference.py after every stamp, the device structures
against a fresh build's, a small frame against the oracle."""
import ctypes as C

import numpy as np
import pytest

import brush_common as bc
import brush_reference as R
from helpers import metallic_palette

pytestmark = pytest.mark.gpu

SRC_DENSE, SRC_BRICKS = (33, 21, 19), (40, 24, 32)


def source_volume(dims, seed):
    W, H, D = dims
    rng = np.random.default_rng(seed)
    return ((rng.random((D, H, W)) < 0.5) * rng.integers(1, 199, (D, H, W))).astype(np.uint8)


def stamps(dims, sdims):
    """(kind, dst_lo, src_lo, size, orient, skip_empty)"""
    W, H, D = dims
    seq = [("orientation %d" % o, (3 + (k % 7) * 8, 2 + (k % 5) * 7, 1 + (k % 6) * 8), (k % 9, k % 5, k % 3), (5, 3, 2), o, bool(k & 1)) for k, o in enumerate(R.ORIENTS)]
    seq += [("negative dst_lo", (-3, -1, -2), (2, 3, 4), (9, 7, 6), 0, False), ("negative dst_lo, turned", (-2, 5, -4), (2, 3, 4), (9, 7, 6), 4 | 3 << 3, True),
            ("the far corner", (W - 4, H - 3, D - 5), (0, 0, 0), (9, 7, 6), 0, False), ("the far corner, turned", (W - 2, H - 6, D - 3), (1, 1, 1), (9, 7, 6), 5 | 6 << 3, True),
            ("wholly outside", (W, 0, 0), (0, 0, 0), (5, 3, 2), 0, False), ("wholly outside, below", (0, -3, 0), (0, 0, 0), (5, 3, 2), 0, False),
            ("a large piece", (5, 4, 3), (0, 0, 0), tuple(min(sdims[a], dims[a] - 6) for a in range(3)), 0, True),
            ("the same again", (5, 4, 3), (0, 0, 0), tuple(min(sdims[a], dims[a] - 6) for a in range(3)), 0, True)]
    return seq


@pytest.mark.parametrize("src_bricks", [False, True], ids=["from-dense", "from-bricks"])
@pytest.mark.parametrize("dst_bricks", [False, True], ids=["to-dense", "to-bricks"])
def test_stamps(vrt, oracle, engine, dst_bricks, src_bricks):
    dims, sdims = (bc.BRICKS if dst_bricks else bc.DENSE_A), (SRC_BRICKS if src_bricks else SRC_DENSE)
    vol = bc.brick_volume(dims, 9) if dst_bricks else bc.dense_volume(dims, 9)
    svol = source_volume(sdims, 10)
    pal = metallic_palette(vrt)
    sky, noise = vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)
    dst = bc.make_scene(vrt, engine, vol, pal, dst_bricks, sky=sky, noise=noise, spare=int((~bc.brick_occupancy(vol)).sum()) if dst_bricks else None)
    src = bc.make_scene(vrt, engine, svol, pal, src_bricks, spare=None)              # a source need not be reserved
    seq = stamps(dims, sdims)
    if dst_bricks != src_bricks:
        seq = seq[:48:6] + seq[48:]                                                    # the 48 orientations on the like pairings
    noops = 0
    for k, (kind, dlo, slo, size, orient, skip) in enumerate(seq):
        what = f"stamp {k} ({kind}) at {dlo} from {slo} size {size} orient {orient} skip {skip}"
        exp, res = R.stamp(vol, dlo, svol, slo, size, orient, skip)
        before = bc.snapshot(vrt, dst, dst_bricks) if res[0] == 0 else None
        got = dst.stamp(dlo, src, slo, size, orient, skip)
        assert got == (res[0], tuple(res[1]), tuple(res[2])), (what, got, res)
        if res[0] == 0:
            noops += 1
            assert bc.same_snapshot(before, bc.snapshot(vrt, dst, dst_bricks)), what
        vol = exp
        assert (bc.whole(dst, dims) == vol).all(), what
        if k % 4 == 3 or k == len(seq) - 1:
            bc.assert_state_equals_fresh(vrt, engine, dst, vol, pal, dst_bricks, what)
        if k % 5 == 4:
            bc.assert_frame_equals_oracle(vrt, oracle, engine, dst, vol, pal, sky, noise, dims, what)
    assert noops >= 3                                                                # the two outside, and the piece stamped twice
    assert (bc.whole(src, sdims) == svol).all()
    dst.destroy(); src.destroy()


@pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
def test_overlapping_self_stamp_copies_the_old_content(vrt, engine, bricks):
    dims = bc.BRICKS if bricks else bc.DENSE_A
    W, H, D = dims
    vol = source_volume(dims, 12)
    vol[:, :, W // 2:] = 0
    pal = metallic_palette(vrt)
    sc = bc.make_scene(vrt, engine, vol, pal, bricks, spare=int((~bc.brick_occupancy(vol)).sum()) if bricks else None)
    for dlo, slo, size, orient, skip in (((13, 5, 6), (10, 5, 6), (30, 20, 25), 0, False), ((10, 3, 7), (10, 5, 6), (30, 20, 25), 0, True),
                                         ((4, 4, 4), (2, 2, 2), (20, 20, 20), 2 | 1 << 3, False), ((0, 0, 0), (0, 0, 0), (W, H, D) if max(dims) <= 512 else (8, 8, 8), 0, False)):
        exp, res = R.stamp(vol, dlo, vol, slo, size, orient, skip)
        got = sc.stamp(dlo, sc, slo, size, orient, skip)
        what = (dlo, slo, size, orient, skip)
        assert got == (res[0], tuple(res[1]), tuple(res[2])), (what, got, res)
        # a copy that read what it had just written would smear the box along the shift
        vol = exp
        assert (bc.whole(sc, dims) == vol).all(), what
        bc.assert_state_equals_fresh(vrt, engine, sc, vol, pal, bricks, str(what))
    sc.destroy()


@pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
def test_a_source_of_three_segments(vrt, engine, bricks):
    """130 x 3 x 3: rows of three segments, the last with two voxels; in every orientation that keeps x, and one that turns it"""
    ddims, sdims = ((152, 16, 24) if bricks else bc.DENSE_B), ((136, 8, 8) if bricks else (131, 5, 4))
    vol = bc.brick_volume((152, 48, 56), 4)[:24, :16, :] .copy() if bricks else bc.dense_volume(ddims, 4)
    svol = source_volume(sdims, 5)
    pal = metallic_palette(vrt)
    dst = bc.make_scene(vrt, engine, vol, pal, bricks, spare=int((~bc.brick_occupancy(vol)).sum()) if bricks else None)
    src = bc.make_scene(vrt, engine, svol, pal, bricks, spare=None)
    for dlo, orient, skip in (((7, 2, 3), 0, False), ((-1, 5, 1), 1 << 3, True), ((19, 0, 6), 1 | 6 << 3, False), ((3, -60, 2), 2, False), ((25, 1, 1), 0, True)):
        exp, res = R.stamp(vol, dlo, svol, (1, 1, 1), (130, 3, 3), orient, skip)
        got = dst.stamp(dlo, src, (1, 1, 1), (130, 3, 3), orient, skip)
        assert got == (res[0], tuple(res[1]), tuple(res[2])), (dlo, orient, skip, got, res)
        vol = exp
        assert (bc.whole(dst, ddims) == vol).all(), (dlo, orient, skip)
        bc.assert_state_equals_fresh(vrt, engine, dst, vol, pal, bricks, f"three segments at {dlo} orient {orient}")
    dst.destroy(); src.destroy()


def test_errors(vrt, engine):
    K, l = vrt._capi, vrt.lib()
    pal = metallic_palette(vrt)
    vol, svol = bc.dense_volume((32, 24, 16), 2), source_volume((20, 10, 600), 3)
    dst, src = vrt.VoxelScene.from_dense(engine, vol, pal), vrt.VoxelScene.from_dense(engine, svol, pal)
    i3, u3 = C.c_int32 * 3, C.c_uint32 * 3

    def rc_of(dlo, slo, size, orient=0, flags=0, d=None):
        r = K.BrushResult()
        rc = l.vrt_scene_stamp(engine.ctx, (d or dst).handle, i3(*dlo), src.handle, i3(*slo), u3(*size), orient, flags, C.byref(r))
        return rc, l.vrt_last_error().decode()
    for args in (((0, 0, 0), (0, 0, 0), (21, 1, 1)), ((0, 0, 0), (-1, 0, 0), (2, 2, 2)), ((0, 0, 0), (0, 9, 0), (2, 2, 2)), ((0, 0, 0), (0, 0, 0), (2, 0, 2)),
                 ((0, 0, 0), (0, 0, 0), (2, 2, 513)), ((0, 0, 0), (0, 0, 0), (2, 2, 2), 6), ((0, 0, 0), (0, 0, 0), (2, 2, 2), 7), ((0, 0, 0), (0, 0, 0), (2, 2, 2), 64),
                 ((0, 0, 0), (0, 0, 0), (2, 2, 2), 0, 2)):
        rc, msg = rc_of(*args)
        assert rc == 1 and "vrt_scene_stamp" in msg, (args, rc, msg)
    assert (bc.whole(dst, (32, 24, 16)) == vol).all()
    assert rc_of((0, 0, 0), (0, 0, 0), (2, 2, 512))[0] == 0                          # 512 is allowed
    vol, _ = R.stamp(vol, (0, 0, 0), svol, (0, 0, 0), (2, 2, 512))
    assert (bc.whole(dst, (32, 24, 16)) == vol).all()
    grid = np.zeros((2, 3, 4), np.uint32); grid[1, 1, 1] = 1
    bs = vrt.VoxelScene.from_bricks(engine, grid, np.full((1, 8, 8, 8), 5, np.uint8), pal)
    rc, msg = rc_of((0, 0, 0), (0, 0, 0), (2, 2, 2), d=bs)
    assert rc == 7 and "vrt_scene_stamp" in msg and "vrt_scene_reserve_bricks" in msg
    assert dst.stamp((1, 1, 1), bs, (8, 8, 8), (8, 8, 8))[0] > 0                      # an unreserved brick scene is a fine source
    vol[1:9, 1:9, 1:9] = 5
    assert (bc.whole(dst, (32, 24, 16)) == vol).all()
    bs.reserve_bricks(1)                                                           # no free slot: a stamp into an empty brick is refused, nothing changes
    snap = bc.snapshot(vrt, bs, True)
    rc, msg = rc_of((0, 0, 0), (0, 0, 0), (2, 2, 2), d=bs)
    assert (rc == 7 and "vrt_scene_reserve_bricks" in msg) or not svol[:2, :2, :2].any()
    assert bc.same_snapshot(snap, bc.snapshot(vrt, bs, True))
    for s in (dst, src, bs):
        s.destroy()
