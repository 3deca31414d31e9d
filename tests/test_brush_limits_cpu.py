"""tests/brush_limits_common.py reaches what it claims -- proved on tests/brush_reference.py (Python integers) alone, without a
device: the rim of every rim case crosses the volume, the products reach the thresholds of the issue (2^59 for the ellipsoid's
left-hand side, 2^57 for the capsule's da2 * L2; the header proves 2^62 and 2^60), each capsule branch decides voxels of the
volume both ways, every no-op changes nothing and every other case something, the 4096-long rows are 4096 long, the brick at
coordinate 511 goes and comes back, and the stamp tables hold the ids, lanes and sides they are named after.  The header itself
(csrc/vrt_brush.h built for the host) is held to the same tables: what the device compiles from the same text."""
import numpy as np
import pytest

import brush_common as bc
import brush_limits_common as L
import brush_native as N
import brush_reference as R
import extents_common as X


@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES, ids=[s[0] for s in L.A_SCENES])
def test_group_a_reaches_the_limits(name, dims, bricks):
    groups = L.group_a(dims)
    assert sorted(groups) == L.A_GROUPS
    largest = {R.ELLIPSOID: 0, R.CAPSULE: 0}
    branches = set()
    radii, modes, capsule_r, rim_axes = set(), set(), set(), set()
    for g in L.A_GROUPS:
        for o, (vol, res) in zip(groups[g], L.a_expected(dims, bricks, g)):
            what = (name, g, o["kind"])
            assert R.shape_ok(o["shape"], o["p"]) and R.mode_ok(o["mode"], o["id"], o["match"]), what
            big, br, any_in, any_out = L.products(o, dims)
            print(what, "reach", big.bit_length() - 1, "changed", res[0], res[2])
            if o["kind"].startswith("no-op"):
                assert res[0] == 0, what
            else:
                assert res[0] >= 1, what
            if o["rim"]:
                assert any_in and any_out, what
            if o["reach"] is not None:
                assert big.bit_length() - 1 == o["reach"], (what, big.bit_length() - 1)         # the value written down in the table
            if o["shape"] == R.ELLIPSOID:
                radii.add(tuple(o["p"][3:6])); modes.add(o["mode"])
                if o["rim"]:
                    rim_axes.add(o["kind"][-2:])
                if tuple(o["p"][3:6]) == (1024, 1024, 1024) and o["rim"]:
                    assert big >= 1 << L.ELLIPSOID_REACH, what
            if o["shape"] == R.CAPSULE:
                capsule_r.add(o["p"][6])
                if g == "capsule-ends":                                             # one end in the volume, the other at the limits
                    assert any(all(v in (L.CMIN, L.CMAX) for v in end) for end in (o["p"][0:3], o["p"][3:6])), what
                else:
                    assert all(v in (L.CMIN, L.CMAX) for a in range(3) for v in (o["p"][a], o["p"][3 + a]) if o["p"][a] != o["p"][3 + a]), what
                branches |= br
            if o["shape"] in largest:
                largest[o["shape"]] = max(largest[o["shape"]], big)
    assert largest[R.ELLIPSOID] >= 1 << L.ELLIPSOID_REACH and largest[R.CAPSULE] >= 1 << L.CAPSULE_REACH, largest
    assert largest[R.ELLIPSOID] < 1 << 62 and largest[R.CAPSULE] < 1 << 60                 # (the header's own bounds)
    assert branches == {(b, v) for b in (1, 2, 3) for v in (False, True)}, branches
    assert radii == set(L.RADII) and modes == {R.SET, R.REPLACE} and capsule_r == {1, 3, 1023, 1024}
    assert rim_axes == {a + s for a in "xyz" for s in "+-"}
    box_lo = {o["p"][0] for o in groups["boxes"]} | {o["p"][2] for o in groups["boxes"]}
    assert box_lo >= {L.INT32_MIN, -L.BIG, -L.BIG + 3, 0, L.INT32_MAX} and all(o["p"][3:6] == [L.BIG] * 3 for o in groups["boxes"])


@pytest.mark.parametrize("name,dims,bricks", L.A_SCENES[:1], ids=[s[0] for s in L.A_SCENES[:1]])
def test_group_a_on_the_header_built_for_the_host(name, dims, bricks):
    """brush_apply_c of tests/native/brush_host.cpp -- csrc/vrt_brush.h in int64 on the host -- gives the tables' volumes and results"""
    for g in L.A_GROUPS:
        vol = L.a_volume(dims, bricks)
        for o, (exp, res) in zip(L.group_a(dims)[g], L.a_expected(dims, bricks, g)):
            rc, got, gres = N.brush(vol, o["shape"], o["mode"], o["p"], o["id"], o["match"])
            assert rc == 0 and (got == exp).all() and (gres[0], list(gres[1]), list(gres[2])) == (res[0], list(res[1]), list(res[2])), (g, o["kind"], gres, res)
            vol = exp.copy()


@pytest.mark.parametrize("dims", [d for d, b in L.B_SCENES if not b], ids=lambda d: "x".join(map(str, d)))
def test_group_b_rows_are_4096_long(dims):
    a = X.long_axis(dims)
    assert dims[a] == 4096 and dims[a] // 8 == 512
    ops = L.limit_ops(dims)
    exp = L.b_expected(dims)
    vol = L.b_volume(dims)
    seen = {}
    for o, (after, res) in zip(ops, exp):
        assert res[0] >= 1, o["kind"]
        occ0, occ1 = bc.brick_occupancy(vol), bc.brick_occupancy(after)
        seen[o["kind"]] = (res, np.moveaxis(occ0, 2 - a, 0).reshape(512), np.moveaxis(occ1, 2 - a, 0).reshape(512))
        vol = after
    assert seen["one voxel at 4095"][0][0] == 1 and seen["one voxel at 4095"][0][1][a] == 4095
    res = seen["semi-axis 1024 on the far face"][0]
    assert res[1][a] == 3584 and res[2][a] == 512
    res = seen["capsule along the whole axis"][0]
    assert res[1][a] == 0 and res[2][a] == 4096                             # 64 segments per row where the axis is x
    res = seen["replace what ADD wrote"][0]
    assert res[0] == seen["capsule along the whole axis"][0][0] and res[2][a] == 4096
    _, before, after = seen["carve brick 511 away"]
    assert before[511] and not after[511]
    _, before, after = seen["carve brick 0 away"]
    assert before[0] and not after[0]
    _, before, after = seen["ADD makes bricks 0 and 511 appear"]
    assert not before[0] and not before[511] and after[0] and after[511]
    for k in (-2, -1):
        dlo, slo, size, orient, skip = ops[k]["stamp"]
        assert size[a] == R.STAMP_MAX_SIDE and exp[k][1][0] >= 1
    assert ops[-2]["stamp"][1][a] == 3584 and ops[-2]["stamp"][3] >> 3 == 1 << a
    assert ops[-1]["stamp"][0][a] + 512 > 4096 and exp[-1][1][1][a] + exp[-1][1][2][a] == 4096       # clipped at the far face, and reaches it


def test_group_c_sources():
    src = L.all_ids_source()
    assert src.shape == L.ALL_IDS_DIMS[::-1] and sorted(src.ravel().tolist()) == list(range(1, 256))
    assert {int(v) >> 5 for v in L.ONE_ID} == {6, 7} and (223 >> 5, 224 >> 5) == (6, 7) and (31 >> 5, 32 >> 5) == (0, 1)
    for vid in L.ONE_ID:
        s = L.slab_source(vid)
        assert set(np.unique(s).tolist()) == {0, vid} and (s[:2] == vid).all() and not s[2:].any()
    for pair in L.BOUNDARY_PAIRS:
        assert set(np.unique(L.pair_source(pair)).tolist()) == {0} | set(pair)
        assert not set(pair) & set(L.NEIGHBOURS) and all(v - 1 in L.NEIGHBOURS or v + 1 in L.NEIGHBOURS for v in pair)
    for lane_x in (63, 64):
        s = L.one_lane_source(lane_x)
        assert int((s >= 200).sum()) == 1 and s[0, 3, lane_x] == 255 and s.shape[2] > 64
    for name, dims, bricks in L.A_SCENES:
        assert not (L.a_volume(dims, bricks) >= 199).any()                  # the destinations hold no metal and none of the ids stamped


@pytest.mark.parametrize("bricks", [False, True], ids=["dense", "bricks"])
@pytest.mark.parametrize("s", [0, 1, 2], ids=["long-x", "long-y", "long-z"])
def test_group_d_stamps(s, bricks):
    svol, slo = L.long_source(s, bricks)
    size = L.long_size(s)
    assert size[s] == 512 and sorted(size) == [2, 3, 512]
    D, H, W = svol.shape
    assert all(slo[a] + size[a] <= (W, H, D)[a] for a in range(3)) and (not bricks or all(v % 8 == 0 for v in (W, H, D)))
    orients = set()
    for t in range(3):
        dims = L.long_dst_dims(t, bricks)
        vol = np.zeros(dims[::-1], np.uint8)
        kinds = set()
        for kind, dlo, orient, skip, noop in L.long_stamps(s, t, dims):
            assert R.orient_ok(orient) and R.stamp_dst_size(orient, size)[t] == 512
            out, res = R.stamp(vol, dlo, svol, slo, size, orient, skip)
            assert (res[0] == 0) == noop, (kind, dlo, res)
            if kind == "one slice":
                assert res[2][t] == 1 and res[1][t] == 0
            if kind == "far face":
                assert res[2][t] == 1 and res[1][t] == dims[t] - 1
            if kind.startswith("perm"):
                assert res[2][t] >= 500                                      # the whole side lands
                orients.add(orient)
            kinds.add(kind.split()[0])
        assert kinds == {"perm", "one", "far", "outside", "INT32_MIN", "INT32_MAX"}
    assert len(orients) == 12 and {o & 7 for o in orients} == set(range(6))      # every permutation, each with the long axis plain and flipped


def test_group_d_large_stamp():
    vol = L.large_volume()
    dlo, slo, size, orient, skip = L.LARGE_STAMP
    assert size[0] * size[1] * size[2] == 512 * 1024 and orient == 2
    out, res = R.stamp(vol, dlo, vol, slo, size, orient, skip)
    assert res[0] > 100000 and all(dlo[a] < slo[a] + size[a] for a in range(3))      # overlapping
    smeared, _ = R.stamp(out, dlo, out, slo, size, orient, skip)
    assert (smeared != out).any()                                               # a copy that read what it wrote would differ
