"""Temporal upsampling without a GPU: the per-pixel definition (csrc/vrt_upsample.h, run over dumped planes by the program
tests/native/upsample_host.cpp) against its numpy float32 restatement (tests/upsample_reference.py) bit for bit, the same
program under ASan + UBSan, the class shares of the sequences, hand-made cases with known answers, the convergence the feature
exists for, the golden fixture that pins the definition, and the C-ABI surface of vrt_upsample."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import reproject_common as rc
import upsample_common as uc
import upsample_reference as ref
from test_reproject_cpu import _plane_frame, _still_push

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "upsample_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_upsample.npz")
PLANES = ("color16", "surface", "resolved8", "motion")


def _build(tmp_path_factory, name, flags):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    return _build(tmp_path_factory, "upsample_host", ["-O2"])


@pytest.fixture(scope="module")
def prog_san(tmp_path_factory):
    """The same program with AddressSanitizer and UndefinedBehaviorSanitizer: a program of its own, nothing loaded into Python."""
    return _build(tmp_path_factory, "upsample_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def run_host(exe, tmp_path, pair, pushes, frames, hist=None, max_history=32, tol_abs=0.5, tol_rel=None, prevs=None, planes=3):
    """csrc/vrt_upsample.h along a sequence, frame k's history feeding frame k + 1 inside the program; the per-frame results in
    the reference's layout.  prevs: the previous push of every frame (default: the frame before, frame 0 its own)."""
    w, h, TW, TH = pair
    inp, outp = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(inp, "wb") as f:
        f.write(struct.pack("<8i2f", w, h, TW, TH, len(frames), max_history, int(hist is not None), planes, tol_abs,
                            -1.0 if tol_rel is None else tol_rel))
        if hist is not None:
            f.write(np.ascontiguousarray(hist[0], np.uint16).tobytes()); f.write(np.ascontiguousarray(hist[1], np.uint32).tobytes())
        for k, (c, p, n) in enumerate(frames):
            prev = prevs[k] if prevs is not None else (pushes[k - 1] if k else pushes[0])
            f.write(bytes(pushes[k])); f.write(bytes(prev))
            f.write(np.ascontiguousarray(c, np.uint8).tobytes()); f.write(np.ascontiguousarray(p, np.float32).tobytes())
            f.write(np.ascontiguousarray(n, np.int8).tobytes())
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    blob, o, out, tn = open(outp, "rb").read(), 0, [], TW * TH
    for _ in frames:
        rcode = struct.unpack_from("<i", blob, o)[0]; o += 4
        if rcode != 0:
            out.append(rcode)
            break
        d = {}
        d["color16"] = np.frombuffer(blob, np.uint16, tn * 4, o).reshape(TH, TW, 4); o += tn * 8
        d["surface"] = np.frombuffer(blob, np.uint32, tn * 4, o).reshape(TH, TW, 4); o += tn * 16
        if planes & 1:
            d["resolved8"] = np.frombuffer(blob, np.uint8, tn * 4, o).reshape(TH, TW, 4); o += tn * 4
        if planes & 2:
            d["motion"] = np.frombuffer(blob, np.float32, tn * 2, o).reshape(TH, TW, 2); o += tn * 8
        out.append(d)
    assert o == len(blob)
    return out


def run_function(exe, tmp_path, mode, rows):
    """upsample_alpha (rows of four float32) or upsample_blend (rows of four uint32) of the header."""
    inp, outp = str(tmp_path / "fin.bin"), str(tmp_path / "fout.bin")
    np.ascontiguousarray(rows, np.float32 if mode == "--alpha" else np.uint32).tofile(inp)
    r = subprocess.run([exe, mode, inp, outp], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    return np.fromfile(outp, np.uint32)


_SEQ = {}


def sequence(vrt, oracle, pair):
    """(seed, pushes, frames) of the moving sequence of a pair, rendered by the oracle once per session."""
    if pair not in _SEQ:
        pushes = uc.pushes_of(vrt, oracle, pair)
        _SEQ[pair] = (uc.seed_of(pair), pushes, rc.oracle_frames(vrt, oracle, uc.seed_of(pair), pushes))
    return _SEQ[pair]


@pytest.mark.parametrize("max_history", uc.MAX_HISTORIES)
@pytest.mark.parametrize("pair", uc.PAIRS, ids=lambda p: "%dx%d-%dx%d" % p)
def test_host_program_matches_numpy_definition(prog, tmp_path, vrt, oracle, pair, max_history):
    """Six frames of floating_cubes(40, seed, count=50) under a strafing, turning camera, jittered with the pair's own phase count
    and rendered by the oracle: color16, surface words, motion bit patterns and resolved8 of the header equal the numpy definition
    in every frame, each side fed its own history."""
    seed, pushes, frames = sequence(vrt, oracle, pair)
    exp = uc.run_definition(pair, pushes, frames, max_history)
    got = run_host(prog, tmp_path, pair, pushes, frames, max_history=max_history)
    for k in range(len(frames)):
        assert ref.same(got[k], exp[k]) == [], (k, ref.same(got[k], exp[k]))
        cnt = got[k]["surface"][..., 3] >> 24
        assert cnt.min() >= 1 and cnt.max() <= min(max_history, k + 1)
    if pair[2] * pair[3] >= 256 and max_history > 1:
        ry, rx = ref.source(*pair)
        assert (cnt > 1).any() and (got[-1]["resolved8"] != frames[-1][0][ry, rx]).any()      # history was used, and it changed the image


def test_same_program_under_asan_and_ubsan(prog_san, tmp_path, vrt, oracle):
    """The program built with -fsanitize=address,undefined (no recovery: any report ends it with a non-zero status) over the
    ragged, the thin and the one-texel pair, with every class of pixel the sequences hold: clean, and the same bits."""
    for pair in ((45, 30, 67, 45), (65, 3, 130, 3), (1, 1, 1, 1)):
        seed, pushes, frames = sequence(vrt, oracle, pair)
        exp = uc.run_definition(pair, pushes, frames, 4)
        got = run_host(prog_san, tmp_path, pair, pushes, frames, max_history=4)
        for k in range(len(frames)):
            assert ref.same(got[k], exp[k]) == [], (pair, k)
    a = run_function(prog_san, tmp_path, "--alpha", [[np.nan, np.inf, 0, 0], [3e38, -3e38, 1, 1]])
    b = run_function(prog_san, tmp_path, "--blend", [[65535, 255, 256, 255], [65535, 255, 0, 255]])
    assert list(a) == [0, 0] and list(b) == [int(ref.blend(65535, 255, 256, 255)), 65535]


@pytest.mark.parametrize("pair", uc.SHARED, ids=lambda p: "%dx%d-%dx%d" % p)
def test_class_shares_and_committed_seed(vrt, oracle, pair):
    """Over the frames that have a history every class -- miss, full, partial, disoccluded, outside, and among the pixels with
    history sampled and carried -- is at least 5 % of the pixels (ratio 1: nothing can be carried, sampled is >= 90 % of the pixels
    with history).  The committed seed is the picker's, which decides on the definition's output alone; the rendered colour does
    not change a pixel's class."""
    seed, sh = uc.pick_scene_seed(vrt, oracle, pair)
    print(f"\n{pair}: scene seed {seed}, shares " + ", ".join(f"{k} {v:.3f}" for k, v in sh.items()))
    assert seed == uc.SEEDS[pair]
    assert min(sh[k] for k in uc.NEEDED) >= 0.05, sh
    if pair[:2] != pair[2:]:
        assert sh["sampled"] >= 0.05 and sh["carried"] >= 0.05, sh
    else:
        assert sh["carried"] == 0.0 and sh["sampled"] >= 0.9 * (sh["full"] + sh["partial"]), sh
    _, pushes, frames = sequence(vrt, oracle, pair)
    assert uc.class_shares(uc.run_definition(pair, pushes, frames)) == sh


# ---- hand-made cases ---------------------------------------------------------------------------------------

HW, HH, HTW, HTH = 8, 4, 16, 8
HPAIR = (HW, HH, HTW, HTH)


def _axis_push(vrt, w=HW, h=HH, pos=(-14.0, 20.2, 20.3), frame=1):
    """A camera that looks along +x: right = (0, 0, -1), up = (0, -1, 0) -- an axis-aligned basis, exact in fp32."""
    p = _still_push(vrt, w, h, pos=pos, yaw=0.0, frame=frame)
    assert list(p.cam_right)[:3] == [0.0, 0.0, -1.0] and list(p.cam_up)[:3] == [0.0, -1.0, 0.0] and p.cam_dir[1] == p.cam_dir[2] == 0.0
    return p


def test_static_camera_has_no_motion_and_one_tap(prog, tmp_path, vrt, oracle):
    """A camera at rest: mv == 0 EXACTLY for every hit, at every ratio and under every jitter of the cycle's first frames (both
    projections are the same arithmetic), so the only tap is the pixel itself with the whole weight 256 * 256, and where it is
    valid in every frame the count goes up by one per frame."""
    for pair in ((48, 32, 96, 64), (56, 37, 96, 64), (32, 21, 96, 64)):
        w, h, TW, TH = pair
        pushes = [_still_push(vrt, w, h, jitter=oracle.jitter(f, w, TW)[1:], frame=f + 1, pos=(20.3, 20.2, -6.0)) for f in range(4)]
        osn = oracle.OracleScene(*rc.scene_of(vrt, 3)[:2])
        pr = oracle.params_from(vrt.VoxelRenderSettings.primary_only().to_c())
        frames = []
        for p in pushes:
            fr = oracle.render(osn, p, pr, planes=["color8", "normal8", "position"])
            frames.append((fr["color8"], fr["position"], fr["normal8"]))
        exp = uc.run_definition(pair, pushes, frames)
        got = run_host(prog, tmp_path, pair, pushes, frames)
        ry, rx = ref.source(*pair)
        for k in range(4):
            assert ref.same(got[k], exp[k]) == []
            assert (got[k]["motion"].view(np.uint32) << 1 == 0).all()                   # +-0, bit for bit
            hit = frames[k][2].view(np.uint32)[..., 0][ry, rx] != 0
            assert 0.1 < hit.mean() < 0.95
            if k:
                # the jittered sample of an edge pixel may show another surface than the pixel's history: then no tap at all
                wt = exp[k]["weight"][hit]
                assert np.isin(wt, (0, 65536)).all() and (wt == 65536).mean() > 0.5 and np.isin(exp[k]["cls"][hit], (1, 3)).all()
            assert ((got[k]["surface"][..., 3] >> 24)[~hit] == 1).all()
        assert ((got[3]["surface"][..., 3] >> 24) == 4).any()


def test_alpha_known_answers(prog, tmp_path):
    """The sample weight: 256 at m = 0, 1 just below one pixel, 0 at exactly one pixel and beyond, 0 for NaN in either coordinate --
    header and restatement alike."""
    one_less = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
    rows = np.array([[5.0, 7.0, 5.0, 7.0],                 # m = 0
                     [5.0 + one_less, 7.0, 5.0, 7.0],      # 5 + (1 - 2^-24) rounds to 6 in fp32: m = 1 exactly
                     [one_less, 0.0, 0.0, 0.0],            # m just below 1
                     [0.0, -one_less, 0.0, 0.0],
                     [6.0, 7.0, 5.0, 7.0],                 # m = 1 exactly
                     [5.0, 8.0, 5.0, 7.0],
                     [5.5, 7.25, 5.0, 7.0],                # m = 0.5
                     [5.0, 7.0 - 1.0 / 256.0, 5.0, 7.0],   # one quantum
                     [np.nan, 7.0, 5.0, 7.0], [5.0, np.nan, 5.0, 7.0], [np.nan, np.nan, 5.0, 7.0], [np.inf, 7.0, 5.0, 7.0],
                     [-1e30, 1e30, 5.0, 7.0]], np.float32)
    want = [256, 0, 1, 1, 0, 0, 128, 255, 0, 0, 0, 0, 0]
    got = run_function(prog, tmp_path, "--alpha", rows)
    assert list(got) == want
    assert list(ref.alpha_of(rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])) == want


def test_blend_known_answers(prog, tmp_path):
    """The blend at the extremes of its numerator -- h = 65535, n = 255 with alpha 0 (the history unchanged) and alpha 256 -- fits
    32 bits and equals the integer formula; alpha 0 carries ANY history unchanged; n = 1, alpha 256 is the colour."""
    rows = [[65535, 255, 0, 255], [65535, 255, 256, 255], [65535, 0, 256, 255], [0, 255, 256, 255], [12345, 77, 0, 7], [12345, 77, 256, 1],
            [12345, 77, 128, 1], [65535, 255, 256, 1], [0, 0, 0, 1]]
    want = [(h * (256 * n - a) + (c << 8) * a + 128 * n) // (256 * n) for h, c, a, n in rows]
    assert max(h * (256 * n - a) + (c << 8) * a + 128 * n for h, c, a, n in rows) == 65535 * 65280 + 32640 < 2 ** 32
    assert want[0] == 65535 and want[4] == 12345 and want[5] == 77 << 8 and want[7] == 65280 and want[6] == (12345 * 128 + (77 << 8) * 128 + 128) // 256
    assert want[1] == 65534 and want[2] == 65278                 # 65535 - 255 / 255 (+ rounding), 65535 - 65535 / 255
    got = run_function(prog, tmp_path, "--blend", rows)
    assert list(got) == want
    r = np.array(rows, np.uint64)
    assert list(ref.blend(r[:, 0], r[:, 1], r[:, 2], r[:, 3])) == want


def _hand_history(vrt, prog, tmp_path, colour=40):
    """Frame 0 of the hand-made pair under the axis-aligned camera, its history recoloured to `colour`.0."""
    cur = _axis_push(vrt)
    col, pos, nrm = _plane_frame(HW, HH, cur, depth=16.0, normal=(-127, 0, 0))
    h0 = run_host(prog, tmp_path, HPAIR, [cur], [(col, pos, nrm)])[0]
    e0 = ref.upsample(*HPAIR, cur, cur, col, pos, nrm)
    assert ref.same(h0, e0) == [] and ((h0["surface"][..., 3] >> 24) == 1).all()
    c16 = h0["color16"].copy(); c16[...] = colour << 8
    return cur, (col, pos, nrm), (c16, h0["surface"].copy())


def test_max_history_one(prog, tmp_path, vrt):
    """max_history = 1: the count stays 1 and the blend is h (256 - alpha) + c alpha over 256.  Every render pixel's point lies on
    its own ray, so the display pixels of a 2 x 2 footprint see it half a display pixel from their centres: alpha = 128."""
    cur, fr, hist = _hand_history(vrt, prog, tmp_path)
    got = run_host(prog, tmp_path, HPAIR, [cur], [fr], hist=hist, max_history=1, tol_abs=1e30)[0]
    exp = ref.upsample(*HPAIR, cur, cur, *fr, hist, 1, tol_abs=1e30)
    assert ref.same(got, exp) == []
    assert ((got["surface"][..., 3] >> 24) == 1).all() and (exp["weight"] == 65536).all()
    assert set(np.unique(exp["alpha"])) <= {128, 129}, np.unique(exp["alpha"])       # floor(m 256) with m = 0.5 -+ rounding
    for a in np.unique(exp["alpha"]):
        want = ((40 << 8) * (256 - int(a)) + (int(fr[0][0, 0, 0]) << 8) * int(a) + 128) // 256
        assert (got["color16"][..., 0][exp["alpha"] == a] == want).all()


def test_previous_position_one_texel_outside_each_edge(prog, tmp_path, vrt):
    """The points lie on a plane 16 voxels in front of the camera, and the previous camera stood 2 voxels to one side: every
    pixel's surface was exactly one display texel further along (2 / 16 of the half-width of 8 texels), so one edge line of the
    frame -- a different one for each of the four directions -- projects one texel outside, finds no tap and starts over, and every
    other pixel takes its neighbour's history."""
    cur, fr, hist = _hand_history(vrt, prog, tmp_path)
    seen = set()
    for axis, delta in ((2, 2.0), (2, -2.0), (1, 2.0), (1, -2.0)):            # world z is -right, world y is -up
        prev = _axis_push(vrt)
        prev.cam_pos[axis] = cur.cam_pos[axis] + delta
        got = run_host(prog, tmp_path, HPAIR, [cur], [fr], hist=hist, tol_abs=1e30, prevs=[prev])[0]
        exp = ref.upsample(*HPAIR, cur, prev, *fr, hist, tol_abs=1e30)
        assert ref.same(got, exp) == []
        cnt = got["surface"][..., 3] >> 24
        comp = 0 if axis == 2 else 1
        mv = got["motion"][..., comp]
        assert np.abs(np.abs(mv) - 1.0).max() < 1e-5 and (np.sign(mv) == np.sign(mv[0, 0])).all() and np.abs(got["motion"][..., 1 - comp]).max() < 1e-5
        line = (slice(None), 0 if mv[0, 0] < 0 else HTW - 1) if comp == 0 else (0 if mv[0, 0] < 0 else HTH - 1, slice(None))
        edge = np.zeros((HTH, HTW), bool); edge[line] = True
        assert (cnt[edge] == 1).all() and (cnt[~edge] == 2).all(), (axis, delta, cnt)
        assert (exp["cls"][edge] == 4).all() and (exp["cls"][~edge] == 1).all()
        ry, rx = ref.source(*HPAIR)
        assert (got["resolved8"][edge] == fr[0][ry, rx][edge]).all()            # the nearest sample, what a blit would show
        seen.add((comp, bool(mv[0, 0] < 0)))
    assert len(seen) == 4


def test_other_normal_code_is_rejected(prog, tmp_path, vrt):
    """A history texel with exactly the right position but another normal code: that pixel alone starts over."""
    cur, fr, hist = _hand_history(vrt, prog, tmp_path)
    surf = hist[1].copy()
    surf[3, 5, 3] = (surf[3, 5, 3] & 0xFF000000) | 0x007F00                  # the +y face's code
    got = run_host(prog, tmp_path, HPAIR, [cur], [fr], hist=(hist[0], surf))[0]
    exp = ref.upsample(*HPAIR, cur, cur, *fr, (hist[0], surf))
    assert ref.same(got, exp) == []
    cnt = got["surface"][..., 3] >> 24
    only = np.zeros((HTH, HTW), bool); only[3, 5] = True
    assert (cnt[only] == 1).all() and (cnt[~only] == 2).all() and exp["cls"][3, 5] == 3
    assert (got["surface"][3, 5, 3] & 0xFFFFFF) == (fr[2].view(np.uint8)[0, 0, 0] | 0)      # rewritten with the pixel's own code


def test_weight_zero_carries_the_history_whole(prog, tmp_path, vrt):
    """A sample that fell far from its pixels (weight 0) and shows another surface than their history -- another normal code, or a
    position out of tolerance: those pixels carry their history texel whole, colour, surface words and count, where the same
    texels under a sample that FELL on them (the neighbouring render pixel) start over."""
    cur, fr, hist = _hand_history(vrt, prog, tmp_path)
    col, pos, nrm = fr
    pos = pos.copy()
    cp = np.array(list(cur.cam_pos)[:3], np.float32)
    pos[1, 2, :3] = cp + np.array([1e-4, 0.0, -1e5], np.float32)                # far to the side: alpha 0, motion 0 (camera at rest)
    pos[2, 5, :3] = cp + np.array([1e-4, 0.0, 1e5], np.float32)
    surf = hist[1].copy()
    surf[..., 3] = (surf[..., 3] & 0xFFFFFF) | (7 << 24)                       # a count the copy must keep
    ry, rx = ref.source(*HPAIR)
    a, b, near = (ry == 1) & (rx == 2), (ry == 2) & (rx == 5), (ry == 1) & (rx == 3)
    surf[a, 3] = (7 << 24) | 0x007F00                                          # another normal code
    surf[near, 3] = (7 << 24) | 0x007F00
    h = (hist[0], surf)
    got = run_host(prog, tmp_path, HPAIR, [cur], [(col, pos, nrm)], hist=h)[0]  # default tolerance: 1e5 voxels away is another surface
    exp = ref.upsample(*HPAIR, cur, cur, col, pos, nrm, h)
    assert ref.same(got, exp) == [], ref.same(got, exp)
    for m in (a, b):
        assert m.sum() == 4 and (exp["alpha"][m] == 0).all() and exp["copied"][m].all() and (got["motion"][m] == 0).all()
        assert (got["surface"][m] == surf[m]).all() and (got["color16"][m] == 40 << 8).all() and (got["resolved8"][m] == 40).all()
    assert exp["copied"].sum() == 8
    assert (exp["alpha"][near] > 0).all() and ((got["surface"][near][:, 3] >> 24) == 1).all() and (got["resolved8"][near] == col[1, 3]).all()
    rest = ~(a | b | near)
    assert ((got["surface"][rest][:, 3] >> 24) == 8).all()


def test_degenerate_bases_and_nan_positions(prog, tmp_path, vrt):
    """A degenerate current (1) or previous (2) basis is reported, not computed; NaN and infinite positions, a point behind the
    camera and the camera's own position give no motion, no history and never a fault -- and both sides agree bit for bit."""
    cur, fr, hist = _hand_history(vrt, prog, tmp_path)
    bad = _axis_push(vrt); bad.cam_right[:] = [0.0, 0.0, 0.0, 0.0]
    assert run_host(prog, tmp_path, HPAIR, [bad], [fr], prevs=[cur]) == [1] and ref.camera(HW, HH, bad) is None
    bad = _axis_push(vrt); bad.cam_dir[0] = float("nan")
    assert run_host(prog, tmp_path, HPAIR, [cur], [fr], prevs=[bad]) == [2]
    col, pos, nrm = fr
    pos = pos.copy()
    cp = np.array(list(cur.cam_pos)[:3], np.float32)
    pos[0, 1, :3] = cp - (pos[0, 1, :3] - cp)              # behind the camera
    pos[1, 2, :3] = cp                                     # l == 0
    pos[2, 3, :3] = np.nan
    pos[3, 4, 0] = np.inf
    pos[3, 5, :3] = cp + np.array([1e-4, 0.0, -1e5], np.float32)
    got = run_host(prog, tmp_path, HPAIR, [cur], [(col, pos, nrm)], hist=hist, tol_abs=1e30)[0]
    exp = ref.upsample(*HPAIR, cur, cur, col, pos, nrm, hist, tol_abs=1e30)
    assert ref.same(got, exp) == [], ref.same(got, exp)
    cnt = got["surface"][..., 3] >> 24
    ry, rx = ref.source(*HPAIR)
    for y, x in ((0, 1), (1, 2), (2, 3), (3, 4)):
        m = (ry == y) & (rx == x)
        assert m.sum() == 4 and (cnt[m] == 1).all() and (got["motion"][m] == 0).all() and (got["resolved8"][m] == col[y, x]).all(), (y, x)
    # 1e-4 in front and 1e5 to the side: the sample fell far outside the frame (alpha 0), and under a camera at rest the pixel
    # was where it is -- motion 0 exactly, its own history carried on unchanged
    m = (ry == 3) & (rx == 5)
    assert (cnt[m] == 2).all() and (got["motion"][m] == 0).all() and (exp["alpha"][m] == 0).all() and (got["color16"][m] == 40 << 8).all()


# ---- convergence -------------------------------------------------------------------------------------------

def test_convergence_beats_the_blit_of_the_mean(vrt, oracle):
    """The reason the feature exists.  A camera at rest in the default orientation (yaw 90, pitch 0: the jitter is a screen shift),
    floating_cubes(40), colour without AO samples and without the denoiser, display 96 x 66, one full jitter cycle at 64 x 44
    (18 frames), 48 x 33 (32) and 32 x 22 (72).  E_up: mean absolute code error of the upsampled resolved image against the
    oracle's unjittered 96 x 66 frame; E_blit: the same for the parent's stand-in, the per-pixel mean of the jittered frames
    rounded as vrt_resolve does and blitted to 96 x 66.  E_up < E_blit at all three ratios; the measured values are printed.

    Measured: 64 x 44: E_up 2.508, E_blit 3.858; 48 x 33: 2.902, 4.924; 32 x 22: 3.896, 6.424.  (With the history DROPPED where a pixel's
    far sample, weight 0, showed another surface than the history -- the first form of step 6 -- a fifth of the pixels of this view
    full of edges restarted every frame and E_up was 4.860 / 5.122 / 6.746, above the blit; such a pixel now carries its history
    texel on whole, which is what weight 0 means.)"""
    TW, TH, seed = 96, 66, 1
    vol = vrt.synthetic.floating_cubes(40, seed=seed)
    pal = vrt.synthetic.default_palette(metallic_ids=range(200, 256))
    osn = oracle.OracleScene(vol, pal, sky=vrt.synthetic.sky_gradient(64, 32), noise=vrt.synthetic.blue_noise_standin(64))
    st = vrt.VoxelRenderSettings(); st.occlusionSettings.numSamples = 0
    pr = oracle.params_from(st.to_c())
    pos = (20.3, 20.2, -14.0)
    truth = oracle.render(osn, _still_push(vrt, TW, TH, pos=pos), pr, planes=["color8"], nthreads=8)["color8"].astype(np.int64)
    measured = []
    for (w, h), cycle in (((64, 44), 18), ((48, 33), 32), ((32, 22), 72)):
        assert oracle.jitter(0, w, TW)[0] == cycle
        pair, hist, acc = (w, h, TW, TH), None, np.zeros((h, w, 4), np.int64)
        prev = None
        for f in range(cycle):
            push = _still_push(vrt, w, h, jitter=oracle.jitter(f, w, TW)[1:], pos=pos, frame=f + 1)
            fr = oracle.render(osn, push, pr, planes=["color8", "normal8", "position"], nthreads=8)
            r = ref.upsample(*pair, push, prev if prev is not None else push, fr["color8"], fr["position"], fr["normal8"], hist)
            hist, prev = (r["color16"], r["surface"]), push
            acc += fr["color8"]
        mean = ((2 * acc + cycle) // (2 * cycle)).astype(np.uint8)
        e_up = float(np.abs(r["resolved8"].astype(np.int64) - truth)[..., :3].mean())
        e_blit = float(np.abs(oracle.blit(mean, TW, TH).astype(np.int64) - truth)[..., :3].mean())
        print(f"\n{w}x{h} -> {TW}x{TH}, {cycle} frames: E_up {e_up:.3f}  E_blit {e_blit:.3f} codes")
        measured.append((w, h, e_up, e_blit))
    assert all(e_up < e_blit for _, _, e_up, e_blit in measured), measured


# ---- golden fixture ----------------------------------------------------------------------------------------

def test_golden_fixture_pins_the_definition(prog, tmp_path, vrt):
    """tests/golden/render_upsample.npz (tests/golden/make_upsample_fixtures.py): the six 48 x 32 frames of the 48 x 32 -> 96 x 64
    sequence and what the definition made of them when the fixture was written -- header and numpy restatement must still give
    exactly that."""
    g = np.load(GOLDEN)
    pair = tuple(int(v) for v in g["pair"])
    assert pair == (48, 32, 96, 64)
    n = int(g["frames"])
    pushes = [vrt._capi.Push.from_buffer_copy(g[f"push{k}"].tobytes()) for k in range(n)]
    frames = [(g[f"color8_{k}"], g[f"position_{k}"], g[f"normal8_{k}"]) for k in range(n)]
    exp = uc.run_definition(pair, pushes, frames, int(g["max_history"]))
    got = run_host(prog, tmp_path, pair, pushes, frames, max_history=int(g["max_history"]))
    for k in range(n):
        want = {name: g[f"{name}_out{k}"] for name in PLANES}
        assert ref.same(got[k], want) == [] and ref.same(exp[k], want) == [], k
    assert ((want["surface"][..., 3] >> 24) == n).any() and ((want["surface"][..., 3] >> 24) == 1).any()


# ---- C-ABI -------------------------------------------------------------------------------------------------

def test_c_abi_surface(vrt):
    """Every VRT_ERR_INVALID of vrt_upsample, all answered before a context or a device is looked at (there is none here); sizes
    from vrt_history_bytes."""
    lib = vrt.lib()
    cap = vrt._capi
    assert "vrt_upsample" in cap.SYMBOLS and hasattr(C.CDLL(cap.LIB_PATH), "vrt_upsample")
    w, h, TW, TH = 48, 32, 96, 64
    cur = _still_push(vrt, w, h)
    st = cap.ReprojectSettings()
    lib.vrt_reproject_settings_default(C.byref(cur), C.byref(st))
    assert np.float32(st.tol_rel) == ref.default_tol_rel(cur, w)              # two RENDER-pixel footprints
    a, b = C.c_size_t(), C.c_size_t()
    assert lib.vrt_history_bytes(TW, TH, C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (TW * TH * 8, TW * TH * 16)
    INVALID, UNSUPPORTED = 1, 7
    err = lambda: lib.vrt_last_error().decode()
    n, tn = w * h, TW * TH
    cur_bytes = 24 * n
    buf = (C.c_uint8 * (cur_bytes + 2 * (a.value + b.value) + 12 * tn + 64))()   # stands for device memory: never dereferenced
    base = (C.addressof(buf) + 63) & ~63
    ctx = C.c_void_p(base)
    col, pos, nrm = base + 16 * n, base, base + 20 * n
    o = base + cur_bytes
    hin = cap.History(o, o + a.value); o += a.value + b.value
    hout = cap.History(o, o + a.value); o += a.value + b.value
    res, mot = o, o + 4 * tn

    def call(ctx=ctx, w=w, h=h, TW=TW, TH=TH, cur=cur, prev=cur, st=st, col=col, pos=pos, nrm=nrm, hin=hin, hout=hout, res=res, mot=mot):
        ref_ = lambda x: C.byref(x) if x is not None else None
        return lib.vrt_upsample(ctx, w, h, TW, TH, ref_(cur), ref_(prev), ref_(st), col, pos, nrm, ref_(hin), ref_(hout), res, mot)

    for kw in (dict(ctx=None), dict(cur=None), dict(prev=None), dict(col=None), dict(pos=None), dict(nrm=None), dict(hout=None),
               dict(hout=cap.History(None, hout.surface)), dict(hin=cap.History(hin.color16, None))):
        assert call(**kw) == INVALID and "NULL" in err(), kw
    assert call(TW=0) == INVALID and call(TH=-1) == INVALID and call(TW=40000) == INVALID and "size" in err()
    assert call(TW=w - 1) == INVALID and "smaller" in err() and call(TH=h - 1) == INVALID and "smaller" in err()
    assert call(TW=16384, TH=16384) == UNSUPPORTED                            # the frame-size limit of vrt_render_geometry, on TW x TH
    other = _still_push(vrt, TW, TH)
    assert call(cur=other) == INVALID and "screen_size" in err() and call(prev=other) == INVALID and "screen_size" in err()
    assert call(w=w + 1) == INVALID and "screen_size" in err()
    for mh in (0, 256):
        assert call(st=cap.ReprojectSettings(mh, 0.5, 0.1)) == INVALID and "max_history" in err()
    for ta, tr in ((-0.5, 0.1), (0.5, -0.1), (float("nan"), 0.1), (0.5, float("inf"))):
        assert call(st=cap.ReprojectSettings(32, ta, tr)) == INVALID and "tolerance" in err(), (ta, tr)
    bad = _still_push(vrt, w, h); bad.cam_right[:] = [0.0, 0.0, 0.0, 0.0]
    assert call(prev=bad) == INVALID and "previous" in err() and "degenerate" in err()
    assert call(cur=bad) == INVALID and "current" in err() and "degenerate" in err()
    bad = _still_push(vrt, w, h); bad.cam_up[1] = float("inf")
    assert call(cur=bad) == INVALID and "degenerate" in err()
    # overlap: history out with history in, with an input, with itself, and the optional outputs likewise -- at DISPLAY extents
    for kw in (dict(hout=hin), dict(hout=cap.History(hin.color16, hout.surface)), dict(hout=cap.History(hout.color16, pos)),
               dict(hout=cap.History(hout.color16, hout.color16)), dict(res=col), dict(res=hout.surface + 64), dict(mot=hin.surface),
               dict(mot=res), dict(res=hout.color16 + 8 * tn - 4), dict(mot=res + 4 * tn - 8), dict(res=nrm + 4 * n - 4)):
        assert call(**kw) == INVALID and "overlap" in err(), kw
    assert call(pos=pos + 4) == INVALID and "aligned" in err()
    assert call(mot=mot + 4) == INVALID and "aligned" in err()
    # the mirrors exist
    assert callable(vrt.UpscalerStage.record_upsampled) and "upsample" in vrt.VoxelRenderer.__init__.__code__.co_varnames
