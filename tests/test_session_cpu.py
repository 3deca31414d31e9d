"""tests/session_common.py reaches what it claims -- proved on the references alone, without a device, for every (volume, seed) of
the table: the session is a function of its seed; every tool, mode and operation occurs; every tool that owns a scratch buffer is
called in large bounds, then in small ones, then in large ones again, and a trim lies between two calls of one tool; on bricks
the planned refusals -- and no other step -- are refused by the model, after slots were freed and taken again, and a step takes
a slot that a step of another tool freed; the metal is written once, by the tool the seed names, where the check frame sees it;
every no-op is one; and the whole model run stays far under the ceiling."""
import json
import time

import numpy as np
import pytest

import brush_common as bc
import brush_reference as BR
import components_reference as CR
import flood_reference as LR
import morph_reference as MR
import session_common as S
import voxelize_reference as VR

CEILING_S = 20.0
IDS = [f"{n}-seed{s}" for n, s in S.TABLE]


@pytest.mark.parametrize("name,seed", S.TABLE, ids=IDS)
def test_the_session_is_a_function_of_its_seed(name, seed):
    dims, bricks = S.VOLUMES[name]
    a, b = S.session(dims, bricks, seed), S.session(dims, bricks, seed)
    assert json.dumps(a) == json.dumps(b)                        # plain data, the same twice
    assert json.dumps(a) != json.dumps(S.session(dims, bricks, seed + 100))
    assert S.session(dims, bricks, seed, 13) == a[:13]           # a prefix is the way to shrink a session
    assert 60 <= len(a) <= 80
    points = [k for k in range(len(a)) if k % S.CHECK_EVERY == S.CHECK_EVERY - 1 or k == len(a) - 1]
    assert 6 <= len(points) <= 10
    assert all(s["tool"] in S.REWRITING + S.READING for s in a)


def test_the_seeds_rotate_the_metal_tool():
    assert {S.METAL_TOOLS[seed % 5] for _, seed in S.TABLE} == set(S.METAL_TOOLS)
    assert len({seed for _, seed in S.TABLE}) == len(S.TABLE) and all(len(S.SEEDS[n]) == 3 for n in S.VOLUMES)


@pytest.mark.parametrize("name,seed", S.TABLE, ids=IDS)
def test_the_table_reaches_what_it_claims(name, seed):
    dims, bricks = S.VOLUMES[name]
    t0 = time.perf_counter()
    S.table_model.cache_clear()
    steps, recs, slots = S.table_model(name, seed)
    took = time.perf_counter() - t0
    print(name, seed, len(steps), "steps, the model took %.2f s" % took)
    assert took < CEILING_S
    by = lambda tool: [(s, r) for s, r in zip(steps, recs) if s["tool"] == tool]
    # every tool, mode and operation
    assert {s["tool"] for s in steps} == set(S.REWRITING + S.READING)
    for tool in S.REWRITING:
        assert sum(r["changed"] > 0 for _, r in by(tool)) >= 2, tool                       # ... and does something, more than once
    assert {s["shape"] for s, _ in by("brush")} == {BR.BOX, BR.ELLIPSOID, BR.CAPSULE}
    assert {s["mode"] for s, _ in by("brush")} == {BR.SET, BR.PAINT, BR.ADD, BR.REPLACE}
    stamps = [s for s, _ in by("stamp")]
    assert {s["src"] for s in stamps} == {"self", "second"} and {s["skip_empty"] for s in stamps if s["src"] == "self"} == {False, True}
    assert len({s["orient"] for s in stamps}) >= 2 and all(BR.orient_ok(s["orient"]) for s in stamps)
    assert {(s["match"], s["conn"]) for s, _ in by("flood")} == {(m, c) for m in (LR.SAME, LR.SOLID) for c in (6, 26)}
    morphs = [s for s, _ in by("morph")]
    assert {s["op"] for s in morphs} == {MR.DILATE, MR.ERODE, MR.OPEN, MR.CLOSE, MR.HOLLOW} and {s["conn"] for s in morphs} == {6, 26}
    assert {s["r"] for s in morphs} >= {1, 2, 3, 8} and {s["border"] for s in morphs} == {False, True}
    assert any(s["bounds"] is None for s in morphs) and any(s["bounds"] is not None and not S.is_large(dims, s["bounds"][1]) for s in morphs)
    filters = [s for s, _ in by("filter")]
    assert any(s["kw"].get("max_voxels") == 1 and s["id"] == 0 for s in filters)                                  # despeckle
    assert any(s["match"] == CR.EMPTY and s["kw"].get("faces_none") == 63 for s in filters)                       # fill_cavities
    assert any(s["kw"].get("keep_largest") for s in filters) and any(s["match"] == CR.SAME and s["id"] != 0 for s in filters)
    vox = [s for s, _ in by("voxelize")]
    assert {s["fill"] for s in vox} == {VR.SURFACE, VR.SOLID, VR.SURFACE | VR.SOLID} and {s["mode"] for s in vox} >= {VR.SET, VR.ADD, VR.PAINT}
    assert any(len(s["triangles"]) == 1 for s in vox) and any(len(s["triangles"]) >= 4 for s in vox)
    # large, small, large for every scratch buffer (a labelling takes the components' buffers as a filter does)
    for buf in sorted(set(S.SCRATCH.values())):
        sizes = ""
        for s in steps:
            if S.SCRATCH.get(s["tool"]) == buf and "extent" in s:
                lo, size = s["extent"]
                sizes += "L" if S.is_large(dims, size) else "s" if S.is_small(lo, size) else "-"
        assert "L" in sizes and "s" in sizes.split("L", 1)[1] and "L" in sizes.split("L", 1)[1].split("s", 1)[1], (buf, sizes)
    # a trim between two calls of one tool; every tool is called again after the first trim or before it
    trims = [k for k, s in enumerate(steps) if s["tool"] == "trim"]
    assert len(trims) >= 2
    for tool in ("morph", "flood", "filter", "voxelize", "brush", "edit", "fill"):
        ks = [k for k, s in enumerate(steps) if s["tool"] == tool]
        assert min(ks) < trims[0] < max(ks), tool
    # the refusals
    refused = [k for k, r in enumerate(recs) if r["refused"]]
    planned = [k for k, s in enumerate(steps) if s.get("refuse")]
    assert refused == planned
    if bricks:
        assert len({steps[k]["tool"] for k in planned}) >= 2
        first = min(planned)
        assert any(a != b for k, a, b in slots.handed if k < first), "no slot was freed and taken again before the refusals"
        assert any(took_ != freed for _, took_, freed in slots.handed), "no step takes a slot another tool freed"
        assert all(0 <= r["free"] for r in recs) and min(r["free"] for r in recs) < bc.BRICK_SPARE < max(r["free"] for r in recs)
    else:
        assert not planned
    # the metal: written once, by the tool the seed names, on the side that faces the camera
    metal = [k for k, s in enumerate(steps) if s.get("metal")]
    assert len(metal) == 1 and steps[metal[0]]["tool"] == S.METAL_TOOLS[seed % 5]
    k = metal[0]
    assert not (recs[k - 1]["vol"] >= 200).any() and recs[k]["changed"] > 0
    for r in recs[k:]:
        assert int((r["vol"][:3] == bc.METAL_ID).sum()) >= dims[0]                        # in the three slices nearest the camera, to the end
    assert not any((np.asarray(s.get("id", 0)) >= 200).any() for j, s in enumerate(steps) if j != k)
    # every no-op is one
    for s, r in zip(steps, recs):
        if s.get("noop"):
            assert r["changed"] == 0 and not r["refused"], s["kind"]
    noops = {s["tool"] for s in steps if s.get("noop")}
    assert noops == set(S.REWRITING)
    # a labelling is followed by a step that reaches the edit pass: the labels go stale
    for k, s in enumerate(steps):
        if s["tool"] == "components":
            nxt = next(j for j in range(k + 1, len(steps)) if steps[j]["tool"] in S.REWRITING)
            assert recs[nxt]["touched"] and steps[nxt]["tool"] != "filter", s["kind"]


def test_the_short_session():
    for dims, bricks, seed in ((bc.DENSE_A, False, 2), (bc.BRICKS, True, 8)):
        steps = S.short_session(dims, bricks, seed)
        assert len(steps) == S.SHORT and {s["tool"] for s in steps} >= set(S.REWRITING)
        vol = bc.brick_volume(dims, 7) if bricks else bc.dense_volume(dims, sum(dims))
        recs, _ = S.run_model(steps, vol, bricks, S.second_volume())
        assert not any(r["refused"] for r in recs)
        for tool in S.REWRITING:
            assert any(r["changed"] > 0 for s, r in zip(steps, recs) if s["tool"] == tool), tool


def test_the_pool_model_is_the_rule_of_expected():
    """brush_common.expected, generalised: the same verdicts for the brush sequence of tests/test_gpu_brush.py"""
    dims = bc.BRICKS
    vol = bc.brick_volume(dims, 7)
    cap = int(bc.brick_occupancy(vol).sum()) + bc.BRICK_SPARE
    seen = []
    for o in bc.brush_sequence(dims, 11):
        free = cap - int(bc.brick_occupancy(vol).sum())
        out, res = BR.brush(vol, o["shape"], o["mode"], o["p"], o["id"], o["match"])
        exp, eres, refused = bc.expected(vol, o, True, free)
        assert refused == (res[0] > 0 and bc.needs_more_slots(vol, out, free))
        assert (exp == (vol if refused else out)).all()
        seen.append(refused)
        vol = exp
    assert any(seen) and not all(seen)
