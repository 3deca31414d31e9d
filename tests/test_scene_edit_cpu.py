"""Scene edits (vrt_scene_edit_box), the part that needs no GPU:
  * the three entry points are declared in include/vrt.h and resolve through vrt.lib();
  * the region arithmetic of csrc/vrt_edit.h against brute force (tests/native/edit_host.cpp): over random small volumes, boxes
    and caps -- boxes at walls and corners, wider than the cap, the whole volume, one voxel; carves, fills and mixtures -- the
    old open-coded fields updated by "recompute R_o reading E only, open cells of Q_o from scans seeded just beyond Q_o's far
    faces, wall clearance for the re-closed cells of Q_o outside R_o, all else untouched" equal the fields of a full rebuild for
    all eight octants, and no byte outside Q_o differs between the two builds;
  * the rule that sends an edit to the full rebuild, on both sides of its threshold."""
import os
import re

import numpy as np
import pytest

from edit_native import HDR, ROOT, edit_host, in_place


def test_entry_points_are_declared_and_resolve(vrt):
    hdr = open(os.path.join(ROOT, "include", "vrt.h")).read()
    for name in ("vrt_scene_edit_box", "vrt_scene_fill_box", "vrt_debug_scene_state"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert getattr(vrt.lib(), name) is not None
    for i, name in enumerate(("VOX", "DF", "OCC1", "OCC2", "OCC3", "CELLS")):
        assert re.search(r"#define VRT_STATE_%s\s+%d\b" % (name, i), hdr), name
        assert getattr(vrt._capi, "STATE_" + name) == i


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_updated_fields_equal_the_rebuilt_ones(seed):
    out = np.zeros(4, np.uint64)
    edit_host().edit_sweep(seed, 100, out.ctypes.data)
    edits, differ, outside, kinds = (int(v) for v in out)
    print(f"seed {seed}: {edits} edits x 8 octants, {differ} fields differ, {outside} bytes changed outside Q_o, kinds {kinds:05b}")
    assert edits == 100 and kinds == 0b11111
    assert differ == 0
    assert outside == 0


def test_cap_matches_the_fields():
    dev = open(os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_device_common.h")).read()
    hdr = open(HDR).read()
    assert re.search(r"#define VRT_DF_CAP (\d+)", dev).group(1) == re.search(r"#define VRT_EDIT_CAP (\d+)", hdr).group(1)


def test_rebuild_rule_both_sides():
    """in place while the cells of the eight R_o together are fewer than 4 W H D and no side exceeds 512"""
    l = edit_host()
    assert in_place(l, (256, 256, 256), (112, 112, 112), (32, 32, 32))        # 8 x 158^3 = 31.6 M < 67.1 M
    assert in_place(l, (256, 256, 256), (0, 0, 0), (32, 32, 32))
    assert in_place(l, (512, 512, 512), (255, 255, 255), (1, 1, 1))
    assert not in_place(l, (256, 256, 256), (0, 0, 0), (256, 256, 256))       # the whole volume
    assert in_place(l, (100, 60, 90), (40, 20, 40), (8, 8, 8))                # (48 + 60)(28 + 40)(48 + 50) = 0.72 M < 2.16 M
    assert not in_place(l, (100, 60, 90), (10, 5, 10), (80, 50, 70))          # (90 + 90)(55 + 55)(80 + 80) = 3.17 M >= 2.16 M
    assert in_place(l, (100, 60, 90), (0, 0, 0), (1, 1, 1))                   # a corner voxel: one octant's R_o is the volume, seven are thin
    assert in_place(l, (4096, 64, 64), (100, 0, 0), (512, 1, 1))
    assert not in_place(l, (4096, 64, 64), (100, 0, 0), (513, 1, 1))          # a side above 512
    # the threshold itself, by the formula: a W x 1 x 1 volume, box of one voxel at x: sum over octants = 4 (x + 1) + 4 (W - x) for W <= 127
    assert in_place(l, (100, 1, 1), (50, 0, 0), (1, 1, 1)) == (4 * 51 + 4 * 50 < 4 * 100)
