"""What tests/test_gpu_launch_shapes.py (on the kernels) and tests/test_launch_shapes_cpu.py (without a device) share: the case tables
of the launch-shape tests and everything about them that numpy can say.

The kernels are held to the oracle elsewhere.  These tables are about the rules AROUND the kernels -- the host loops that cut one call
into several launches, and the rules that size a launch from the frame -- at values the other tests never reach: the second chunk of
a batch, a ring slot that is used again, a denoiser segment that is longer than the minimum.

  BATCH_SIZES, poses()         vrt_render_geometry_batch / _slots: 8 slots in the kernel arguments, 256 in a table, more in a second launch
  COPY_SIZES, copy_shards()    vrt_*_rows_batch / vrt_*_halo_batch: 64 images per launch
  PAIR_CASES, VER_CASES,       k_denoise_pair / k_denoise_ver: the rows of a segment, stated per case and recomputed from
  SHARD_PAIR_CASE              pair_segments() / ver_segments() by the CPU test
  TAGS_SEQ, tags_sequence()    the ten launches of the "tags_async" test (tests/stream_common.py runs them on other streams too)
"""
import numpy as np

# ---- A. frame batches --------------------------------------------------------------------------------------------------------------

MAX_BATCH, MAX_TABLE, TAB_RING = 8, 256, 4          # VRT_MAX_BATCH, VRT_MAX_TABLE (csrc/vrt_internal.h), vrt_ctx::kTabRing (csrc/vrt_host.h)
BATCH_SIZES = (8, 9, 256, 257, 301)                 # the last slot in the arguments, the first in a table, a full table, a second launch of 1 and of 45
ORACLE_FRAMES = (0, 7, 8, 255, 256)                 # ... and the last frame of each batch
BATCH_DIMS = (32, 32, 32)
BATCH_RES = (48, 32)
SLOTS_N, SLOTS_RES, SLOTS_RANKS, SLOTS_STRIP = 260, (48, 40), 3, 16      # 40 rows: strips of 16, 16 and 8 rows, one per rank
RING_LAUNCHES, RING_N = 6, 9
POISON = 0xA5


def poses(n, dims=BATCH_DIMS):
    """n different camera poses (pos, yaw, pitch, frame, jitter) around a volume: every frame of a batch has its own, and every
    seventh looks away from the volume (all sky: a launch whose tags say "nothing to trace")."""
    W, H, D = dims
    out = []
    for f in range(n):
        a = 0.37 * f
        pos = (W / 2.0 + 0.9 * W * np.cos(a) + 0.013 * f, H / 2.0 + 0.21 + 0.3 * H * np.sin(0.11 * f), D / 2.0 + 0.9 * D * np.sin(a))
        yaw = np.degrees(np.arctan2(D / 2.0 - pos[2], W / 2.0 - pos[0])) + 7.0 * np.sin(0.5 * f)      # towards the centre, give or take
        if f % 7 == 3:
            yaw += 180.0
        out.append(dict(pos=tuple(float(v) for v in pos), yaw=float(yaw), pitch=float(-12.0 * np.sin(0.11 * f)), frame=f,
                        jitter=(float(0.5 * np.sin(1.3 * f)), float(0.5 * np.cos(0.7 * f)))))
    return out


def launches_of_batch(n):
    """[(first frame, frames)] of the launches render_many cuts n frames into, and whether each reads its slots from a table."""
    return [(f0, min(MAX_TABLE, n - f0), min(MAX_TABLE, n - f0) > MAX_BATCH) for f0 in range(0, n, MAX_TABLE)]


# ---- B. strip and halo copies ------------------------------------------------------------------------------------------------------

ROWS_BATCH = 64                                     # VRT_ROWS_BATCH (csrc/vrt_internal.h)
COPY_SIZES = (64, 65, 130)
COPY_W, COPY_H, COPY_STRIP, COPY_HALO = 40, 50, 16, 3
_COPY_CYCLE = ((0, 2), (1, 2), (0, 3), (1, 3), (2, 3))      # (rank, nranks): 50 rows are 4 strips, 2 per rank at most for 2 and for 3 ranks


def copy_shards(n):
    """(rank, nranks) of image i: a cycle of five, so image 64 + k never has the shard of image k (64 % 5 = 4), and every image of
    a call packs into the same number of rows (one launch per 64 images)."""
    return [_COPY_CYCLE[i % len(_COPY_CYCLE)] for i in range(n)]


def mixed_shards(n):
    """Shards whose packed buffers differ in rows from image to image: 1, 2, 3 and 4 ranks (50 rows: 50, 32, 32 and 16 packed rows;
    halo rows: 1, 2, 2 and 1 strips' worth)."""
    cyc = ((0, 4), (0, 2), (0, 1), (2, 3), (3, 4), (1, 2), (1, 4))
    return [cyc[i % len(cyc)] for i in range(n)]


def own_row_map(H, rank, nranks, strip_rows, distributed):
    """packed row -> frame row of vrt_pack_rows / vrt_unpack_rows (-1: padding); one rank: the frame itself."""
    return distributed.packed_row_map(H, rank, nranks, strip_rows)


def halo_map(H, rank, nranks, strip_rows, halo, direction, distributed):
    if nranks <= 1:                                 # one strip, the whole frame: its first / last `halo` rows
        return np.arange(halo) if direction < 0 else np.arange(H - halo, H)
    return distributed.halo_row_map(H, rank, nranks, strip_rows, halo, direction)


# ---- C. segment lengths ------------------------------------------------------------------------------------------------------------
# RESTATEMENT of the two rules launch_denoise_pass (csrc/vrt_denoise.hip) sizes its launches by, in Python, for whole frames and for a rank's strips:
# strip_ext is the height of what one walk covers (the frame; sharded: strip_rows + 2 * extend), total all rows of the launch (the
# frame; sharded: strip_ext * local strips).  The rules themselves are denoise_plan's (csrc/vrt_denoise_plan.h), and
# tests/test_launch_shapes_cpu.py holds this restatement to that function, on every row below and over a sweep of frames.  If the rule
# changes there, change it here, and choose the cases below anew: they are only worth their time while they produce the lengths
# their rows state.

def pair_segments(W, total, strip_ext, R, pair_wgs):
    """(seg_rows, segments per strip, rows of the last segment) of a k_denoise_pair launch."""
    strips = (W + (64 - 2 * R) - 1) // (64 - 2 * R)
    wgs = max(1, (pair_wgs if pair_wgs > 0 else 4096 // R) // strips)
    if pair_wgs <= 0:
        wgs = max(wgs, (total + 47) // 48)
    seg = max(2 * R, ((total + wgs - 1) // wgs + R - 1) // R * R)
    segs = (strip_ext + seg - 1) // seg
    return seg, segs, strip_ext - (segs - 1) * seg


def ver_segments(W, total, strip_ext, pass0):
    """The same of a k_denoise_ver launch (pass0: the blur, whose ring holds the colour plane only)."""
    strips = (W + 63) // 64
    wgs = max(1, (2048 if pass0 else 1024) // strips)
    seg = max(8, ((total + wgs - 1) // wgs + 3) & ~3)
    segs = (strip_ext + seg - 1) // seg
    return seg, segs, strip_ext - (segs - 1) * seg


def tap_offsets(iterations, step):
    """R of every pass: i * stepWidth + 1 (integral in every case here)."""
    return [int(i * step + 1) for i in range(iterations)]


class PairCase:
    """Two passes -- k_denoise_p0, then ONE weighted pass with tap offset R = step + 1 through k_denoise_pair -- with the context option
    denoise_pair_wgs = pair_wgs.  seg_rows, last: what the launch of the weighted pass is meant to walk in."""

    def __init__(self, W, H, R, pair_wgs, seg_rows, last, what):
        self.W, self.H, self.R, self.pair_wgs, self.seg_rows, self.last, self.what = W, H, R, pair_wgs, seg_rows, last, what
        self.iterations, self.step = 2, float(R - 1)


def _pair_cases():
    c = []
    # 130 x 117: three column strips for every R; the knob is a multiple of 3, a third of it the segments per strip asked for
    for R, rows in ((2, ((0, 4, 1, "minimum"), (60, 6, 3, "3R"), (9, 40, 37, "long"), (3, 118, 117, "single"))),
                    (3, ((0, 6, 3, "minimum"), (39, 9, 9, "3R"), (9, 39, 39, "long"), (3, 117, 117, "single"))),
                    (4, ((0, 8, 5, "minimum"), (30, 12, 9, "3R"), (9, 40, 37, "long"), (3, 120, 117, "single"))),
                    (5, ((0, 10, 7, "minimum"), (24, 15, 12, "3R"), (9, 40, 37, "long"), (3, 120, 117, "single")))):
        c += [PairCase(130, 117, R, pw, seg, last, what) for pw, seg, last, what in rows]
    # A segment near 48 rows whose last one is shorter than R: seg_rows * workgroups >= rows by the rule, so the last segment is
    # short only by what the rounding to a multiple of R adds up to over all the others -- no frame of 117 rows has such a length.
    # The shortest frames that have one, per R (and the same frame at the minimum, for the counts to be compared with):
    for R, H, pw, seg in ((2, 925, 66, 44), (3, 631, 45, 45), (4, 441, 33, 44), (5, 361, 27, 45)):
        c += [PairCase(130, H, R, 0, 2 * R, H - (H - 1) // (2 * R) * (2 * R), "minimum"), PairCase(130, H, R, pw, seg, 1, "near48-short-last")]
    return c


PAIR_CASES = _pair_cases()
PAIR_LENGTHS = ("minimum", "3R", "long", "single", "near48-short-last")


class VerCase:
    """k_denoise_ver alone (denoise_pair = 0, denoise_p0 = 0).  No knob: the segment follows from the frame, 1024 workgroups (pass 0:
    2048) over the column strips, so wide and low frames.  passes: (R, seg_rows, last) per pass, pass 0 first."""

    def __init__(self, W, H, iterations, step, mode, passes):
        self.W, self.H, self.iterations, self.step, self.mode, self.passes = W, H, iterations, step, mode, passes

    @property
    def id(self):
        return f"{self.W}x{self.H}-i{self.iterations}w{self.step:g}-m{self.mode}"


VER_CASES = [
    # 16384 columns: 256 strips, 4 workgroups per strip (pass 0: 8)
    VerCase(16384, 37, 3, 1.0, 0, [(1, 8, 5), (2, 12, 1), (3, 12, 1)]),           # last segment of ONE row, shorter than R = 2 and 3
    VerCase(16384, 49, 3, 2.0, 0, [(1, 8, 1), (3, 16, 1), (5, 16, 1)]),           # ... than R = 3 and 5
    VerCase(16384, 65, 2, 0.0, 0, [(1, 12, 5), (1, 20, 5)]),                      # pass 0 in segments of 12; a weighted pass with R = 1
    VerCase(16384, 37, 3, 2.0, 1, [(1, 8, 5), (3, 12, 1), (5, 12, 1)]),           # the as-shipped taps
    VerCase(16384, 65, 3, 1.0, 1, [(1, 12, 5), (2, 20, 5), (3, 20, 5)]),
    VerCase(16384, 37, 2, 0.0, 1, [(1, 8, 5), (1, 12, 1)]),                       # ... with the tap offset at run time (RT = 0)
]


class ShardPairCase:
    """Sharded, extended strips of 64 rows and more: k_denoise_pair with the segment count forced.  rank -> (seg_rows, last)."""
    W, H, nranks, strip_rows, iterations, step, R, pair_wgs = 117, 200, 2, 64, 2, 2.0, 3, 21
    per = 64                                        # strip_rows + 2 * 0: the weighted pass is the last one
    local_strips = {0: 2, 1: 2}                     # rows 0-63 and 128-191; rows 64-127 and 192-199
    seg_rows, last = 21, 1                          # 64 = 3 * 21 + 1


# ---- D. the tolerance kernels ------------------------------------------------------------------------------------------------------

FAST_SIZES = ((200, 120), (70, 13))
FAST_STEPS = (2.0, 1.0)
FAST_ITERATIONS = (2, 3, 4)
FAST_SHARD = (70, 50, 2, 16, 2, 2.0)                # W, H, ranks, strip rows, iterations, step: k_denoise_lds<.., FAST> (extended strips of 16 rows)
# VRT_DENOISE_FAST through the verified pass' cheap half, k_denoise_ver<.., FLAG = false> ("denoise_pair" = 0; the as-shipped taps take it
# anyway): three column strips, five segments of 8 rows.  (iterations, step) -> the tap offsets of the weighted passes, which are the
# kernel's RT: 2, 3 and 5 at compile time, 4 at run time (RT = 0)
FAST_VER_SIZE = (130, 37)
FAST_VER_SETTINGS = {(3, 1.0): (2, 3), (3, 2.0): (3, 5), (2, 3.0): (4,)}


# ---- E. "tags_async" --------------------------------------------------------------------------------------------------------------
# Ten launches on a scene whose tile tags differ from pose to pose: facing the volume, facing away, grazing it, a sharded launch, a
# batch of 11 through the table (the tag kernel waits for the upload), a larger batch (the tag buffer is allocated anew), single
# frames again.  A batch is (first, last) of poses(TAGS_POOL, TAGS_DIMS).

TAGS_DIMS, TAGS_RES, TAGS_AO = (48, 48, 48), (96, 64), 2
TAGS_CUBES = dict(seed=3, count=40)                 # vrt.synthetic.floating_cubes(48, **TAGS_CUBES)
TAGS_POSES = {"facing": dict(frame=1), "away": dict(yaw=270.0, frame=2),
              "grazing": dict(pos=(-0.6, 24.2, -20.0), yaw=90.0, frame=3, jitter=(0.25, -0.25)),
              "above": dict(pos=(24.3, 70.0, 10.0), yaw=90.0, pitch=-60.0, frame=4)}
TAGS_POOL = 25
TAGS_SHARD = (1, 2, 16)                             # rank, nranks, strip_rows
TAGS_SEQ = (("single", "facing", None), ("single", "away", None), ("single", "grazing", None), ("single", "facing", TAGS_SHARD),
            ("batch", (0, 11), None), ("batch", (11, 25), None), ("single", "above", None), ("single", "grazing", None),
            ("batch", (3, 14), None), ("single", "facing", None))


def tags_sequence(vrt, camera_push):
    """[(kind, [push blocks], shard triple or None)] of TAGS_SEQ; camera_push: tests/helpers.py's."""
    pool = [camera_push(vrt, TAGS_DIMS, TAGS_RES, **p) for p in poses(TAGS_POOL, TAGS_DIMS)]
    named = {k: camera_push(vrt, TAGS_DIMS, TAGS_RES, **p) for k, p in TAGS_POSES.items()}
    return [(kind, [named[what]] if kind == "single" else pool[what[0]:what[1]], shard) for kind, what, shard in TAGS_SEQ]
