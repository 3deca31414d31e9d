"""The table of tests/stream_common.py without a device: it names every function of the C-ABI that takes a context -- in a step or
in NOT_STREAMED, never both --, its steps exist, its shapes are small, and its edits do what their comments say."""
import os
import re

import numpy as np

import launch_shapes_common as lsc
import scene_reference as R
import stream_common as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ctx_functions(header_text):
    """Names of the vrt_* functions whose first parameter is a vrt_ctx*."""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    return sorted(set(re.findall(r"\b(vrt_\w+)\s*\(\s*(?:const\s+)?vrt_ctx\s*\*", text)))


def _header():
    with open(os.path.join(ROOT, "include", "vrt.h")) as f:
        return f.read()


def coverage_errors(functions, stepped, not_streamed):
    bad = [f"{f}: in no step of a case and not in NOT_STREAMED" for f in functions if f not in stepped and f not in not_streamed]
    bad += [f"{f}: in a step AND in NOT_STREAMED" for f in functions if f in stepped and f in not_streamed]
    bad += [f"{f}: in NOT_STREAMED but no function of include/vrt.h takes a context under that name" for f in not_streamed if f not in functions]
    return bad


def test_every_context_function_is_streamed_or_excused():
    fns = ctx_functions(_header())
    assert len(fns) > 50 and "vrt_render_geometry" in fns and "vrt_scene_info" not in fns and "vrt_ctx_create" not in fns
    stepped = {st.name for _, st in sc.all_steps()}
    assert coverage_errors(fns, stepped, sc.NOT_STREAMED) == []
    assert all(isinstance(r, str) and r.strip() and "\n" not in r for r in sc.NOT_STREAMED.values())
    # the check itself: a function that is dropped from both places, or put into both, is reported
    victim = "vrt_scene_reserve_bricks"
    assert victim in stepped
    assert coverage_errors(fns, stepped - {victim}, sc.NOT_STREAMED) == [f"{victim}: in no step of a case and not in NOT_STREAMED"]
    assert coverage_errors(fns, stepped, dict(sc.NOT_STREAMED, **{victim: "x"})) == [f"{victim}: in a step AND in NOT_STREAMED"]
    assert coverage_errors(fns + ["vrt_new_stage"], stepped, sc.NOT_STREAMED) != []


def test_every_step_is_a_function_of_the_binding(vrt):
    for case, st in sc.all_steps():
        assert st.name in vrt._capi.SYMBOLS, (case.id, st.name)
    assert [c.id for c in sc.CASES] == sorted({c.id for c in sc.CASES}, key=[c.id for c in sc.CASES].index)       # ids are unique
    for c in sc.CASES:
        assert c.steps and set(c.not_on) <= set(sc.KINDS) and all(c.not_on.values()), c.id
        outs = [st.args["out"] for st in c.setup + c.steps if "out" in st.args]
        assert len(outs) == len(set(outs)), (c.id, "the expected values are keyed by the outputs' names")
        assert 1 <= c.behind <= sum(st.name not in sc.AFTER_THE_WAIT for st in c.steps), c.id
    # the helper-stream cases are warmed so that no launch of the sequence waits: every step is held behind the stall
    for c in (sc.E_TAGS0, sc.E_TAGS2, sc.H, sc.I):
        assert c.behind == sum(st.name not in sc.AFTER_THE_WAIT for st in c.steps), c.id
    for c in (sc.E_TAGS0, sc.E_TAGS2):
        warm = [st for st in c.setup if st.name == "vrt_render_geometry_batch"]
        assert len(warm) == 2 and all(st.args["tags_poses"][1] - st.args["tags_poses"][0] == 14 for st in warm)      # both tag buffers, the largest batch
        assert c.setup[-1].name == "vrt_ctx_set_option"                # set last: the sequence's first launch makes the tag stream


def test_shapes_stay_small():
    for case, st in sc.all_steps():
        for key in ("res", "target"):
            if key in st.args and not case.imported:
                w, h = st.args[key]
                assert 0 < w * h <= 1 << 15, (case.id, st)
        if "volume" in st.args:
            assert max(sc.DIMS[st.args["volume"]]) <= 64, (case.id, st)
    assert {c.id for c in sc.CASES if c.imported} == {"E-ring", "E-tags0", "E-tags2", "I"}
    assert sc.COPY_N == lsc.ROWS_BATCH + 1 and sc.I.steps[0].args["res"] == (lsc.COPY_W, lsc.COPY_H)
    assert lsc.BATCH_RES[0] * lsc.BATCH_RES[1] <= 1 << 15 and lsc.TAGS_RES[0] * lsc.TAGS_RES[1] <= 1 << 15
    assert sc.STALL_BYTES == 1 << 30 and sc.STALL_PASSES >= 16


def test_the_imported_sequences_are_the_launch_shape_tests(vrt):
    ring = [st for st in sc.E_RING.steps if st.name == "vrt_render_geometry_batch"]
    assert len(ring) == lsc.RING_LAUNCHES > lsc.TAB_RING and all(st.args["poses"][1] - st.args["poses"][0] == lsc.RING_N > lsc.MAX_BATCH for st in ring)
    for case in (sc.E_TAGS0, sc.E_TAGS2):
        assert [("single" if st.name == "vrt_render_geometry" else "batch") for st in case.steps] == [k for k, _, _ in lsc.TAGS_SEQ]
        assert [st.args.get("tags_pose", st.args.get("tags_poses")) for st in case.steps] == [w for _, w, _ in lsc.TAGS_SEQ]
    from helpers import camera_push
    seq = lsc.tags_sequence(vrt, camera_push)
    assert len(seq) == 10 and len(seq[5][1]) > len(seq[4][1]) > lsc.MAX_BATCH and seq[3][2] == (1, 2, 16)
    assert [len(p) for _, p, _ in seq] == [1, 1, 1, 1, 11, 14, 1, 1, 11, 1]


def test_the_edits_do_what_the_table_says(vrt):
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    metal = pal[:, 4] > 0
    # B: no metallic voxel before the edit_box, one after; the fill lies in the corner (0, 0, 0)
    steps = sc.B.setup + sc.B.steps
    k = next(i for i, st in enumerate(steps) if st.name == "vrt_scene_edit_box")
    before, after = sc.volume_after(vrt, steps, k)["s"], sc.volume_after(vrt, steps, k + 1)["s"]
    assert not metal[before].any() and metal[after].any() and (before != after).any()
    fill = next(st for st in steps if st.name == "vrt_scene_fill_box")
    assert tuple(fill.args["lo"]) == (0, 0, 0)
    # C: the first fill makes empty bricks occupied, within the reservation; the edit empties a brick; the second fill occupies one
    steps = sc.C.steps
    occ = [R.brick_occupancy(sc.volume_after(vrt, steps, i + 1)["s"]) for i in range(len(steps))]
    at = {name: [i for i, st in enumerate(steps) if st.name == name] for name in ("vrt_scene_fill_box", "vrt_scene_edit_box", "vrt_scene_reserve_bricks")}
    f1, f2 = at["vrt_scene_fill_box"]
    e, = at["vrt_scene_edit_box"]
    r, = at["vrt_scene_reserve_bricks"]
    assert r < f1 < e < f2
    appeared = int((occ[f1] & ~occ[f1 - 1]).sum())
    assert 0 < appeared <= steps[r].args["extra"] and not (~occ[f1] & occ[f1 - 1]).any()
    assert int((~occ[e] & occ[e - 1]).sum()) == 1 and not (occ[e] & ~occ[e - 1]).any()
    assert int((occ[f2] & ~occ[f2 - 1]).sum()) == 1 and not (~occ[f2] & occ[f2 - 1]).any()
    assert sc.DIMS["cubes48"] == (48, 48, 48) and not occ[0].all()
    # apply_box against a loop
    vol = np.zeros((4, 5, 6), np.uint8)
    out = sc.apply_box(vol, (1, 2, 3), 7, (2, 3, 1))
    assert out.sum() == 7 * 6 and (out[3, 2:5, 1:3] == 7).all()
    ids = sc.box_ids(("random", 3, (3, 2, 2), 1.0, None))
    assert ids.shape == (2, 2, 3) and (sc.apply_box(vol, (0, 0, 0), ids)[:2, :2, :3] == ids).all()
