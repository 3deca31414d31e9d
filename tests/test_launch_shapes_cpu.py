"""The case tables of tests/launch_shapes_common.py, checked without a device: every case really produces the launch shape its row
states -- by the Python restatement of launch_denoise_pass' rules there --, every pass of a case is one the library verifies
(vrt_denoise_guard needs no device), and the batch and copy tables cross the chunk sizes they are about.  A change to a rule that
would put every case back at the minimum segment fails here instead of passing silently on the GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_plan_native as dpn
import denoise_shard_common as dsc
import launch_shapes_common as lsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxel-raytracing_amd", "csrc")
GUARD_MAX = 0.02                                    # kDenGuardMax: the largest guard a pass is verified with


def _define(name, text):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)", text)
    assert m, name
    return int(m.group(1))


def test_chunk_sizes_are_the_librarys():
    internal = open(os.path.join(CSRC, "vrt_internal.h")).read()
    assert _define("VRT_MAX_BATCH", internal) == lsc.MAX_BATCH
    assert _define("VRT_MAX_TABLE", internal) == lsc.MAX_TABLE
    assert _define("VRT_ROWS_BATCH", internal) == lsc.ROWS_BATCH
    m = re.search(r"kTabRing\s*=\s*(\d+)", open(os.path.join(CSRC, "vrt_host.h")).read())
    assert m and int(m.group(1)) == lsc.TAB_RING


def test_batch_sizes_cross_every_boundary():
    shapes = {n: lsc.launches_of_batch(n) for n in lsc.BATCH_SIZES}
    assert shapes[8] == [(0, 8, False)] and shapes[9] == [(0, 9, True)]                       # arguments / table
    assert shapes[256] == [(0, 256, True)] and shapes[257] == [(0, 256, True), (256, 1, False)]
    assert any(len(s) == 2 and s[1][2] for s in shapes.values())                                # a second launch that reads a table too
    assert len(lsc.launches_of_batch(lsc.SLOTS_N)) == 2
    assert lsc.RING_LAUNCHES > lsc.TAB_RING + 1 and lsc.RING_N > lsc.MAX_BATCH                  # a slot of the ring is used a second time
    # every frame its own pose, some of them looking away
    ps = lsc.poses(max(lsc.BATCH_SIZES))
    assert len({(p["pos"], p["yaw"], p["jitter"]) for p in ps}) == len(ps)
    # the slots' frames: every rank of the split owns rows, the last strip is a partial one
    H = lsc.SLOTS_RES[1]
    own = [dsc.owned_rows(H, r, lsc.SLOTS_RANKS, lsc.SLOTS_STRIP) for r in range(lsc.SLOTS_RANKS)]
    assert all(len(o) for o in own) and len(own[-1]) < lsc.SLOTS_STRIP and sum(len(o) for o in own) == H


def test_copy_tables(vrt):
    D = vrt.distributed
    H, S = lsc.COPY_H, lsc.COPY_STRIP
    assert lsc.COPY_SIZES == (lsc.ROWS_BATCH, lsc.ROWS_BATCH + 1, 2 * lsc.ROWS_BATCH + 2)
    sh = lsc.copy_shards(max(lsc.COPY_SIZES))
    assert all(sh[k] != sh[k + lsc.ROWS_BATCH] for k in range(len(sh) - lsc.ROWS_BATCH))
    assert all(sh[k] != sh[k + 2 * lsc.ROWS_BATCH] for k in range(len(sh) - 2 * lsc.ROWS_BATCH))
    assert len({n for _, n in sh}) > 1 and len({r for r, _ in sh}) > 1
    # one launch per 64 images: every image packs into the same number of rows, own rows and halo rows alike
    assert len({D.packed_rows(H, n, S) for _, n in sh}) == 1 and len({D.max_local_strips(H, n, S) for _, n in sh}) == 1
    # image 64 + k read with the shard of image k would move other rows
    for k in range(len(sh) - lsc.ROWS_BATCH):
        a, b = sh[k], sh[k + lsc.ROWS_BATCH]
        assert not np.array_equal(D.packed_row_map(H, a[0], a[1], S), D.packed_row_map(H, b[0], b[1], S))
        for d in (-1, 1):
            assert not np.array_equal(D.halo_row_map(H, a[0], a[1], S, lsc.COPY_HALO, d), D.halo_row_map(H, b[0], b[1], S, lsc.COPY_HALO, d))
    # the mixed table: packed buffers of different heights side by side
    mixed = lsc.mixed_shards(20)
    assert len({len(lsc.own_row_map(H, r, n, S, D)) for r, n in mixed}) >= 3
    assert len({len(lsc.halo_map(H, r, n, S, lsc.COPY_HALO, 1, D)) for r, n in mixed}) >= 2
    assert lsc.halo_map(H, 0, 1, S, 3, -1, D).tolist() == [0, 1, 2] and lsc.halo_map(H, 0, 1, S, 3, 1, D).tolist() == [47, 48, 49]


def _guard(vrt, iterations, step, mode, p):
    ds = vrt._capi.DenoiserSettings()
    vrt.lib().vrt_denoiser_settings_default(C.byref(ds))
    ds.iterations, ds.step_width, ds.mode = iterations, step, mode
    g = C.c_float()
    vrt._capi.check(vrt.lib().vrt_denoise_guard(C.byref(ds), p, C.byref(g)))
    return float(g.value)


def test_pair_cases_produce_the_stated_segments(vrt):
    by_R = {}
    for c in lsc.PAIR_CASES:
        assert lsc.tap_offsets(c.iterations, c.step) == [1, c.R]
        seg, segs, last = lsc.pair_segments(c.W, c.H, c.H, c.R, c.pair_wgs)
        assert (seg, last) == (c.seg_rows, c.last), (c.W, c.H, c.R, c.pair_wgs, seg, segs, last)
        assert seg % c.R == 0 and (segs - 1) * seg + last == c.H
        assert _guard(vrt, c.iterations, c.step, 0, 1) <= GUARD_MAX              # the weighted pass is verified: k_denoise_pair takes it
        by_R.setdefault(c.R, {})[c.what] = (c, seg, segs, last)
    assert sorted(by_R) == [2, 3, 4, 5]
    for R, d in by_R.items():
        assert set(d) == set(lsc.PAIR_LENGTHS)
        assert d["minimum"][1] == 2 * R and d["3R"][1] == 3 * R
        assert d["single"][2] == 1 and d["single"][1] >= d["single"][0].H
        assert d["long"][2] >= 2 and d["long"][1] > 6 * R
        assert abs(d["near48-short-last"][1] - 48) <= 4 and 0 < d["near48-short-last"][3] < R and d["near48-short-last"][2] >= 2
    # the counts of redone pixels are compared between the cases of one frame: every frame has at least two segment lengths
    frames = {}
    for c in lsc.PAIR_CASES:
        frames.setdefault((c.W, c.H, c.R), set()).add(c.seg_rows)
    assert all(len(v) >= 2 for v in frames.values())


def test_ver_cases_produce_the_stated_segments(vrt):
    lengths, short, Rs = set(), False, set()
    for c in lsc.VER_CASES:
        assert c.W * c.H < 1_400_000
        assert lsc.tap_offsets(c.iterations, c.step) == [p[0] for p in c.passes]
        for i, (R, seg_rows, last) in enumerate(c.passes):
            seg, segs, l = lsc.ver_segments(c.W, c.H, c.H, i == 0)
            assert (seg, l) == (seg_rows, last), (c.id, i, seg, segs, l)
            assert seg % 4 == 0 and (segs - 1) * seg + l == c.H
            assert i == 0 or _guard(vrt, c.iterations, c.step, c.mode, i) <= GUARD_MAX
            if i > 0 and seg > 8:
                lengths.add(seg); Rs.add(R)
                short |= l < R
    assert len(lengths) >= 3 and short and Rs >= {1, 2, 3, 5}
    assert any(c.mode == 1 and any(p[1] > 8 for p in c.passes[1:]) for c in lsc.VER_CASES)       # the as-shipped taps
    assert any(c.passes[0][1] > 8 for c in lsc.VER_CASES)                                        # pass 0


def test_sharded_pair_case_produces_the_stated_segments(vrt):
    c = lsc.ShardPairCase
    assert lsc.tap_offsets(c.iterations, c.step)[-1] == c.R and dsc.reaches(c.iterations, c.step)[-1] == c.R
    assert c.per == c.strip_rows and c.per >= 64                                   # the pair kernel is taken
    for rank in range(c.nranks):
        n_local = len(dsc.strips(c.H, rank, c.nranks, c.strip_rows))
        assert n_local == c.local_strips[rank]
        seg, segs, last = lsc.pair_segments(c.W, n_local * c.per, c.per, c.R, c.pair_wgs)
        assert (seg, last) == (c.seg_rows, c.last) and segs >= 2 and last < c.R
        assert seg != lsc.pair_segments(c.W, n_local * c.per, c.per, c.R, 0)[0]   # not what the launch would choose by itself
    assert _guard(vrt, c.iterations, c.step, 0, 1) <= GUARD_MAX


# ---- the tables held to the code: denoise_plan (csrc/vrt_denoise_plan.h), the function launch_denoise_pass launches by, built for the host
# (tests/native/denoise_plan_host.cpp) and given what vrt_denoise gives it (tests/denoise_plan_native.py: passes) ---------------------------

def _segments(q, strip_ext):
    return q.seg_rows, q.segs, strip_ext - (q.segs - 1) * q.seg_rows


def test_restated_segment_rules_are_the_plans_on_every_table_row(vrt):
    for c in lsc.PAIR_CASES:
        for mode in (0, dpn.DENOISE_FAST):                                          # (the GPU test runs both)
            p0, w = dpn.passes(vrt, c.W, c.H, c.iterations, c.step, mode, options={"denoise_pair_wgs": c.pair_wgs})
            assert p0.name == "k_denoise_p0" and w.name == "k_denoise_pair" and w.pair_R == c.R and w.FLAG == (mode == 0)
            assert _segments(w, c.H) == lsc.pair_segments(c.W, c.H, c.H, c.R, c.pair_wgs)
            assert (w.seg_rows, _segments(w, c.H)[2]) == (c.seg_rows, c.last)
    for c in lsc.VER_CASES:
        ps = dpn.passes(vrt, c.W, c.H, c.iterations, c.step, c.mode, options={"denoise_pair": 0, "denoise_p0": 0})
        assert len(ps) == len(c.passes)
        for i, (q, (R, seg_rows, last)) in enumerate(zip(ps, c.passes)):
            assert q.name == "k_denoise_ver" and (q.R, q.SHIPPED, q.PASS0, q.FLAG) == (R, c.mode & 1, int(i == 0), 1), (c.id, i)
            assert _segments(q, c.H) == lsc.ver_segments(c.W, c.H, c.H, i == 0)
            assert (q.seg_rows, _segments(q, c.H)[2]) == (seg_rows, last)
    c = lsc.ShardPairCase
    for rank in range(c.nranks):
        w = dpn.passes(vrt, c.W, c.H, c.iterations, c.step, 0, options={"denoise_pair_wgs": c.pair_wgs}, shard=(rank, c.nranks, c.strip_rows))[-1]
        assert w.name == "k_denoise_pair" and w.pair_R == c.R and w.grid_y == w.segs * c.local_strips[rank]
        assert _segments(w, c.per) == lsc.pair_segments(c.W, c.local_strips[rank] * c.per, c.per, c.R, c.pair_wgs)
        assert (w.seg_rows, _segments(w, c.per)[2]) == (c.seg_rows, c.last)


def test_restated_segment_rules_are_the_plans_everywhere():
    """pair_segments / ver_segments against the plan over frames the tables do not hold: W = 1, W one below, at and one above a multiple
    of the strip width (64 - 2 R; 64 for k_denoise_ver), heights below 2 R, whole frames and a rank's extended strips, the knob off and forced."""
    n = {"k_denoise_pair": 0, "k_denoise_ver": 0}
    for R in range(1, 6):
        ow = 64 - 2 * R
        Ws = sorted({1, ow - 1, ow, ow + 1, 3 * ow - 1, 3 * ow, 3 * ow + 1, 63, 64, 65, 191, 192, 193, 4097, 16384})
        Hs = sorted({1, 2, 3, 2 * R - 1, 2 * R, 2 * R + 1, 8, 9, 47, 48, 49, 117, 361, 925, 2160})
        shapes = [(H, H, dict()) for H in Hs]                                      # (total rows, strip height, the shard)
        shapes += [(local * (strip + 2 * ext), strip + 2 * ext, dict(nranks=2, strip_rows=strip, n_local_strips=local, extend=ext))
                   for strip in (16, 64, 80) for ext in (0, 3, 8) for local in (1, 2, 3)]
        for W in Ws:
            for total, per, shard in shapes:
                H = total if not shard else 2 * shard["strip_rows"] * shard["n_local_strips"] - 5
                for pw in (0, 1, 3, 21, 60, 4096):
                    q = dpn.plan(W, H, float(R), False, pair_wgs=pw, **shard)
                    pair = R >= 2 and (not shard or per >= 64)
                    assert q.name == ("k_denoise_pair" if pair else "k_denoise_ver"), (W, H, R, pw, shard)
                    want = lsc.pair_segments(W, total, per, R, pw) if pair else lsc.ver_segments(W, total, per, False)
                    assert _segments(q, per) == want, (W, H, R, pw, shard)
                    n[q.name] += 1
                for pass0 in (False, True):
                    q = dpn.plan(W, H, float(R), pass0, no_pair=1, no_p0=1, **shard)
                    assert q.name == "k_denoise_ver" and q.PASS0 == pass0 and _segments(q, per) == lsc.ver_segments(W, total, per, pass0), (W, H, R, pass0, shard)
                    n[q.name] += 1
    assert min(n.values()) > 5000, n


# What the `path` label of a case in denoise_shard_common.cases() (and the comment above it there) claims: the kernel family of pass 0
# and of a weighted pass.  f: the facts of the pass -- R its tap offset (integral: f.integral), per the height of an extended strip,
# the case's options.  The conditions (per >= 64, per a multiple of 4, R <= 5) are the plan's own thresholds written once more, as the case
# comments state them: a threshold changed in the plan fails here because this table copies the number, not because the table knows
# better.  It is the cases' claim held to the code, not a second derivation of the rule; the same holds for `pair` in the sweep above.
def _ver(f): return "k_denoise_ver"
def _literal(f): return "k_denoise_lds" if f.per % 4 == 0 else "k_denoise"           # (R <= 5 in every such case)


PATHS = {
    # label:         (pass 0,                                                        a weighted pass)
    "p0-ver":        ("k_denoise_p0",                                                _ver),
    "pair":          ("k_denoise_p0",                                                lambda f: "k_denoise_pair" if f.per >= 64 else "k_denoise_ver"),
    "pair-p0-off":   (lambda f: "k_denoise_p0" if f.p0 else "k_denoise_ver",         lambda f: "k_denoise_pair" if f.pair and f.per >= 64 else "k_denoise_ver"),
    "shipped":       ("k_denoise_ver",                                               _ver),
    "literal":       (_literal,                                                      _literal),
    "bilinear":      ("k_denoise_p0",                                                lambda f: "k_denoise_ver" if f.integral else "k_denoise"),
    "guard":         ("k_denoise_p0",                                                _literal),
    "edges":         ("k_denoise_p0",                                                _ver),
    "halo-gt-strip": ("k_denoise_p0",                                                lambda f: "k_denoise_ver" if f.R <= 5 else "k_denoise"),
}


class _Facts:
    pass


def test_case_labels_name_the_kernels_the_plan_takes(vrt):
    taken = {}
    for c in dsc.CASES:
        assert set(c.options) <= {"denoise_verified", "denoise_pair", "denoise_p0", "denoise_packed"}
        if c.guard_too_large:
            assert dpn.guard(vrt, c.iterations, c.step, c.mode, c.phis, 1) > GUARD_MAX
        ext = dsc.reaches(c.iterations, c.step)
        for rank in range(c.nranks):
            ps = dpn.passes(vrt, c.W, c.H, c.iterations, c.step, c.mode, c.phis, c.options, (rank, c.nranks, c.strip_rows))
            assert len(ps) == (c.iterations if dsc.strips(c.H, rank, c.nranks, c.strip_rows) else 0)
            for i, q in enumerate(ps):
                f = _Facts()
                sw = np.float32(i) * np.float32(c.step) + np.float32(1.0)
                f.R, f.integral, f.per = int(sw), float(sw) == int(sw), c.strip_rows + 2 * sum(ext[i + 1:])
                f.pair, f.p0 = c.options.get("denoise_pair", 1), c.options.get("denoise_p0", 1)
                claim = PATHS[c.path][min(i, 1)]
                want = claim if isinstance(claim, str) else claim(f)
                assert q.name == want, (c.id, rank, i, q.instantiation, want)
                assert q.SHIPPED == c.mode or q.name in ("k_denoise", "k_denoise_p0", "k_denoise_pair")
                taken.setdefault(c.path, set()).add((min(i, 1), q.name) + ((q.pair_R,) if q.name == "k_denoise_pair" else ()))
    assert set(taken) == set(PATHS)
    # ... and each label reaches what it is for
    assert {(1, "k_denoise_pair", R) for R in (2, 3, 4, 5)} <= taken["pair"] and (1, "k_denoise_ver") in taken["pair"]
    assert {(0, "k_denoise_ver"), (0, "k_denoise_p0"), (1, "k_denoise_pair", 3), (1, "k_denoise_ver")} <= taken["pair-p0-off"]
    assert taken["literal"] == {(i, k) for i in (0, 1) for k in ("k_denoise", "k_denoise_lds")}
    assert (1, "k_denoise") in taken["bilinear"] and (1, "k_denoise_lds") in taken["guard"] and (1, "k_denoise") in taken["halo-gt-strip"]


# The arms of launch_denoise_pass' switch: every instantiation of the denoiser kernels (profiles/denoise_plan_kernel_digest.txt lists
# the same 43), as (family, template arguments).
INSTANTIATIONS = (
    [("k_denoise", inf) for inf in (0, 1)]
    + [("k_denoise_lds", inf, sh, fast, packed) for sh in (0, 1) for inf, fast, packed in ((0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0))]
    + [("k_denoise_fast", sh, th) for sh in (0, 1) for th in (8, 16)]
    + [("k_denoise_ver", sh, 1, rt, 1) for sh in (0, 1) for rt in (1, 0)]
    + [("k_denoise_ver", sh, fl, rt, 0) for sh in (0, 1) for fl in (0, 1) for rt in (2, 3, 5, 0)]
    + [("k_denoise_pair", fl, R) for fl in (0, 1) for R in (2, 3, 4, 5)]
    + [("k_denoise_p0", 1)])

# Instantiations that no case table of the GPU tests reaches, and why.  No development switch guards these two: vrt_denoise cannot launch
# them at all.  PASS0 is the blur, all three phis +inf, and RT = 0 with it a tap offset other than 1.  Pass 0 has the offset 0 * stepWidth + 1 = 1;
# a later pass has phis of +inf only if the caller passes +inf, and then its guard is +inf too and the pass is not verified
# (test_a_blur_with_another_tap_offset_is_never_verified).  The parent has the same two arms; which instantiations exist is not this table's to change.
NOT_REACHED = dict(
    [(("k_denoise_ver", sh, 1, 0, 1), "a verified pass with phis of +inf and a tap offset above 1: vrt_denoise makes none") for sh in (0, 1)])


def test_a_blur_with_another_tap_offset_is_never_verified(vrt):
    inf = float("inf")
    for mode in (0, 1, 2, 3):
        for step in (0.0, 1.0, 2.0, 3.0, 4.0, 0.5):
            for i in range(1, 10):
                assert dpn.guard(vrt, 10, step, mode, (inf, inf, inf), i) > GUARD_MAX
            for q in dpn.passes(vrt, 130, 37, 10, step, mode, phis=(inf, inf, inf))[1:]:
                assert q.PHI_INF and q.name in ("k_denoise", "k_denoise_lds")


def test_fast_ver_rows_take_the_cheap_half_of_the_verified_kernel(vrt):
    W, H = lsc.FAST_VER_SIZE
    seen = set()
    for (iterations, step), offsets in lsc.FAST_VER_SETTINGS.items():
        assert tuple(lsc.tap_offsets(iterations, step)[1:]) == offsets
        for mode in (0, 1):
            ps = dpn.passes(vrt, W, H, iterations, step, mode | dpn.DENOISE_FAST, options={"denoise_pair": 0})
            assert ps[0].instantiation == (("k_denoise_lds", 1, 1, 0, 0) if mode else ("k_denoise_p0", 1))      # pass 0: exact kernels
            for q, R in zip(ps[1:], offsets):
                assert q.instantiation == ("k_denoise_ver", mode, 0, R if R in (2, 3, 5) else 0, 0) and q.R == R
                assert _segments(q, H) == lsc.ver_segments(W, H, H, False) and q.grid_x > 1 and q.segs > 1
                seen.add(q.instantiation)
    assert len(seen) == 8


def _table_plans(vrt):
    """[(table, plans of one vrt_denoise call)] of every call the GPU tests make from the case tables"""
    out = []
    for c in dsc.CASES:
        out += [("dsc.cases", dpn.passes(vrt, c.W, c.H, c.iterations, c.step, c.mode, c.phis, c.options, (rank, c.nranks, c.strip_rows))) for rank in range(c.nranks)]
    for c in lsc.PAIR_CASES:
        out += [("PAIR_CASES", dpn.passes(vrt, c.W, c.H, c.iterations, c.step, mode, options={"denoise_pair_wgs": c.pair_wgs})) for mode in (0, dpn.DENOISE_FAST)]
    for c in lsc.VER_CASES:
        out.append(("VER_CASES", dpn.passes(vrt, c.W, c.H, c.iterations, c.step, c.mode, options={"denoise_pair": 0, "denoise_p0": 0})))
    c = lsc.ShardPairCase
    out += [("ShardPairCase", dpn.passes(vrt, c.W, c.H, c.iterations, c.step, 0, options={"denoise_pair_wgs": c.pair_wgs}, shard=(rank, c.nranks, c.strip_rows)))
            for rank in range(c.nranks)]
    for W, H in lsc.FAST_SIZES:
        for step in lsc.FAST_STEPS:
            for mode in (0, 1):
                for iterations in (1,) + tuple(lsc.FAST_ITERATIONS):
                    out += [("FAST_*", dpn.passes(vrt, W, H, iterations, step, mode | dpn.DENOISE_FAST, options={"denoise_verified": 0, "denoise_th16": th16}))
                            for th16 in (0, 1)]
    W, H, N, S, iterations, step = lsc.FAST_SHARD
    out += [("FAST_SHARD", dpn.passes(vrt, W, H, iterations, step, mode | dpn.DENOISE_FAST, options={"denoise_verified": 0}, shard=(rank, N, S)))
            for mode in (0, 1) for rank in range(N)]
    W, H = lsc.FAST_VER_SIZE
    out += [("FAST_VER", dpn.passes(vrt, W, H, iterations, step, mode | dpn.DENOISE_FAST, options={"denoise_pair": 0}))
            for mode in (0, 1) for iterations, step in lsc.FAST_VER_SETTINGS]
    return out


def test_every_instantiation_is_reached_by_a_case_table(vrt):
    assert len(set(INSTANTIATIONS)) == len(INSTANTIATIONS) == 43
    reached = {q.instantiation for _, ps in _table_plans(vrt) for q in ps}
    assert reached <= set(INSTANTIATIONS)
    assert set(INSTANTIATIONS) - reached == set(NOT_REACHED), sorted(set(INSTANTIATIONS) - reached)


def test_the_switchs_arms_are_the_objects_kernels():
    """INSTANTIATIONS against the two committed kernel listings (tools/kernel_digest.py over the objects of this commit and of its parent:
    equal line for line) and against the arms of the switch in csrc/vrt_denoise.hip."""
    here, parent = (open(os.path.join(ROOT, "profiles", n)).read() for n in ("denoise_plan_kernel_digest.txt", "denoise_plan_parent_kernel_digest.txt"))
    assert here == parent
    listed = set()
    for m in re.finditer(r"^_ZN3vrt\d+(k_denoise\w*?)I((?:L[bi]\d+E)+)EEvNS_13DenoiseParamsE", here, re.M):
        listed.add((m.group(1),) + tuple(int(a) for a in re.findall(r"L[bi](\d+)E", m.group(2))))
    assert listed == set(INSTANTIATIONS)
    arms = re.findall(r"case denoise_key\((\w+)((?:, \d+)+)\):\s+hipLaunchKernelGGL\(\((k_denoise\w*)<", open(os.path.join(CSRC, "vrt_denoise.hip")).read())
    assert sorted((k,) + tuple(int(a) for a in args.split(", ")[1:]) for _, args, k in arms) == sorted(INSTANTIATIONS)


def test_the_plan_under_the_sanitizers(tmp_path):
    """The stand-alone program of tests/native/denoise_plan_host.cpp, built with -fsanitize=address,undefined: the sweep of small
    frames, a rank's strips, and the largest frames (32768 a side; W * H up to 2^28 - 1, the verified form's bound).  Exit status 0, and
    the checksums of the unsanitized shared-library build."""
    lines = dpn.run_main_program(str(tmp_path / "denoise_plan_main_san"))
    assert [l[0] for l in lines] == list(range(dpn.BLOCKS))
    for block, plans, checksum in lines:
        n = C.c_uint64()
        assert dpn.lib().denoise_plan_block_c(block, C.byref(n)) == checksum and n.value == plans and plans > 10000
