"""Edits of brick scenes (vrt_scene_reserve_bricks, then vrt_scene_edit_box), the part that needs no GPU:
  * the entry point and the three brick selectors of vrt_debug_scene_state are declared in include/vrt.h, exported by
    libvrt_hip.so and known to _capi;
  * the region arithmetic of csrc/vrt_brick_edit.h against brute force (tests/native/brick_edit_host.cpp): over random brick
    lattices, contents and boxes a build by the definitions gives the fine bytes, the coarse bytes, the open bits and the packed
    entries before and after the edit; every changed byte lies in the region the header names (F, R_o, Q_o), an edit that changes
    no occupancy changes nothing at brick level, and the in-place update of the coarse fields equals the build;
  * the rule that sends an edit to the full build path, on both sides."""
import os
import re
import subprocess

import numpy as np
import pytest

from brick_edit_native import ROOT, brick_edit_host, in_place, spans


def test_entry_point_and_selectors(vrt):
    hdr = open(os.path.join(ROOT, "include", "vrt.h")).read()
    assert re.search(r"\bint\s+vrt_scene_reserve_bricks\s*\(", hdr)
    assert vrt.lib().vrt_scene_reserve_bricks is not None
    for i, name in enumerate(("VOX", "DF", "OCC1", "OCC2", "OCC3", "CELLS", "BENTRY", "BPOOL", "BFINE")):
        assert re.search(r"#define VRT_STATE_%s\s+%d\b" % (name, i), hdr), name
        assert getattr(vrt._capi, "STATE_" + name) == i
    so = os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "libvrt_hip.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout
    assert re.search(r"\bT vrt_scene_reserve_bricks\b", syms)
    assert hasattr(vrt.VoxelScene, "reserve_bricks")
    mirror = open(os.path.join(ROOT, "voxel-raytracing_amd", "host", "voxels.hpp")).read()
    assert "reserveBricks" in mirror and "vrt_scene_reserve_bricks" in mirror


def test_cap_matches_the_build():
    api = open(os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_api_scene.hip")).read()
    hdr = open(os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_brick_edit.h")).read()
    assert re.search(r"#define VRT_BRICK_EDIT_CAP (\d+)", hdr).group(1) == "16"
    assert re.search(r"launch_build_df\(occ, \(int\)nbx, \(int\)nby, \(int\)nbz, s->bcoarse\.get\(\), cstride, tmp0, tmp1, c->stream, VRT_BRICK_EDIT_CAP\)", api)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_changed_bytes_lie_in_the_named_regions(seed):
    out = np.zeros(14, np.uint64)
    brick_edit_host().brick_edit_sweep(seed, 120, out.ctypes.data)
    (trials, fine_out, occ_out, coarse_out, open_out, entry_out, unchanged_diff, update_diff, changed, full, with_fine, kinds, emptied,
     created) = (int(v) for v in out)
    print(f"seed {seed}: {trials} edits ({with_fine} with fine bytes), {changed} changed some occupancy ({emptied} emptied, {created} created a brick; "
          f"{full} by the rule's full build); outside their regions: fine {fine_out}, occupancy {occ_out}, coarse {coarse_out}, open {open_out}, "
          f"entries {entry_out}; brick-level changes without an occupancy change {unchanged_diff}; in-place fields that differ {update_diff}")
    assert trials == 120 and with_fine == 60 and kinds == 0b111111
    assert changed >= 30 and trials - changed >= 20 and emptied >= 10 and created >= 10
    assert 2 <= full <= changed - 2                               # the rule was exercised on both sides
    assert fine_out == 0 and occ_out == 0                         # F, T
    assert coarse_out == 0                                        # R_o
    assert open_out == 0 and entry_out == 0                       # Q_o
    assert unchanged_diff == 0
    assert update_diff == 0


def test_spans():
    l = brick_edit_host()
    s = spans(l, (64, 40, 8), (100, 7, 63), (29, 2, 1))           # voxels 100..128, 7..8, 63
    assert s["T"] == [(12, 17), (0, 2), (7, 8)]
    assert s["F"] == [(11, 18), (0, 3), (6, 8)]
    assert s["R"][0] == [(12, 32), (0, 17), (7, 8)]               # octant (-, -, -): grown towards +
    assert s["R"][7] == [(0, 17), (0, 2), (0, 8)]                 # octant (+, +, +): grown towards -
    assert s["E"][3] == [(0, 32), (0, 17), (0, 8)]
    assert s["Q"][0] == [(12, 64), (0, 40), (7, 8)]
    assert s["Q"][7] == [(0, 17), (0, 2), (0, 8)]
    assert s["Q"][1] == [(0, 17), (0, 40), (7, 8)]


def test_rebuild_rule_both_sides():
    """in place while the bricks of the eight R_o together are fewer than 4 nbx nby nbz"""
    l = brick_edit_host()
    assert in_place(l, (256, 256, 256), (1000, 1000, 1000), (32, 32, 32))     # 8 x 20^3 bricks against 67 M
    assert in_place(l, (256, 256, 256), (0, 0, 0), (1, 1, 1))
    assert not in_place(l, (256, 256, 256), (0, 0, 0), (2048, 2048, 2048))
    # a lattice no wider than the cap: R_o reaches the walls, the sum over the octants is the product over the axes of (nb + n)
    assert in_place(l, (12, 8, 11), (40, 30, 40), (8, 8, 8))                  # 13 * 9 * 12 = 1404 < 4224
    assert not in_place(l, (12, 8, 11), (8, 8, 8), (80, 48, 72))              # 22 * 14 * 20 = 6160 >= 4224
    assert in_place(l, (4, 1, 1), (8, 0, 0), (8, 8, 8)) == ((4 + 1) * 2 * 2 < 4 * 4)
    assert in_place(l, (4, 4, 4), (8, 8, 8), (8, 8, 8)) == (5 ** 3 < 4 * 64)
    assert in_place(l, (4, 4, 4), (8, 8, 8), (16, 16, 16)) == (6 ** 3 < 4 * 64)
    assert not in_place(l, (4, 4, 4), (4, 4, 4), (20, 20, 20))                # 7^3 = 343 >= 256
