"""One vrt_scene through every rewriting tool in turn, held to the model of tests/session_common.py: box edits, brushes, stamps,
flood fill, morphology, component filters and mesh voxelization on the same scene, on large bounds, then small ones, then large
ones again, with reads, measurements, ray queries, vrt_scene_memory and vrt_scene_trim in between.

After every rewriting step the tool's result equals its reference's, the whole volume read back equals the model and, on bricks,
every brick lies in the slot the model's stack gives it; a no-op or a refused step leaves every byte of every structure alone.
After every reading step the answer equals the reference's on the model and the structures are unchanged.  At every ninth step and
at the end the structures equal a fresh build's, a small frame equals the oracle's (with the metal seen once a tool has written
it), and the count planes equal those of the same frame on a fresh scene.  vrt_scene_memory never falls between two calls that
are not vrt_scene_trim and is back at its first value after a trim, with two things set apart that are no scratch.  A dense scene's
list of occupied cells is allocated at its exact length and counted so (csrc/vrt_api_scene.hip, build_cell_list): it grows and
shrinks with the volume, so its four bytes per cell of STATE_CELLS are taken out of every figure; its content is held to a fresh
build's.  And an edit drops the count planes' fields (csrc/vrt_api_edit.hip, scene_edit_locked): what a check-point frame added is
what the next edit may take away.  Every session runs twice from scratch for identical structures, pool slots included."""
import ctypes as C

import numpy as np
import pytest

import brush_common as bc
import session_common as S
import stream_common as sc_
from helpers import compare_planes, metallic_palette
from ray_query_common import oracle_records, planes_differ, query_rays

pytestmark = pytest.mark.gpu

NAMES = bc.GB + ["hit_id", "rays_total"]
COUNT_PLANES = ("steps_primary", "steps_total", "rays_total")
MAX_STEPS = 512


def same_end(a, b, bricks):
    """two snapshots of two scenes that went the same way: every byte of a dense scene; of a brick scene every entry (so every
    brick in the same pool slot), the cell list in its order, and the ids and clearances of every slot an entry points to -- a
    slot that was never taken holds whatever the allocation held"""
    if not bricks:
        return bc.same_snapshot(a, b)
    (ea, pa, fa, ca), (eb, pb, fb, cb) = a, b
    if not (ea.shape == eb.shape and (ea == eb).all() and ca.shape == cb.shape and (ca == cb).all() and pa.shape == pb.shape and fa.shape == fb.shape):
        return False
    ptr = (ea & bc.PTR).astype(np.int64)
    used = ptr[(ptr != 0) & (ptr != 0xFFFFFF)] - 1
    return bool((pa[used] == pb[used]).all() and (fa[used] == fb[used]).all())


class Player:
    """a scene and the model's records side by side"""
    def __init__(self, vrt, oracle, engine, vol, bricks, what, textures=True):
        self.vrt, self.oracle, self.engine, self.bricks, self.what = vrt, oracle, engine, bricks, what
        self.dims = (vol.shape[2], vol.shape[1], vol.shape[0])
        self.pal = metallic_palette(vrt)
        self.sky, self.noise = (vrt.synthetic.sky_gradient(64, 32), vrt.synthetic.blue_noise_standin(64)) if textures else (None, None)
        self.sc = bc.make_scene(vrt, engine, vol, self.pal, bricks, sky=self.sky, noise=self.noise)
        self.second = vrt.VoxelScene.from_dense(engine, S.second_volume(), self.pal)
        self.base = self.last = self.held()                      # before the first tool call; of a brick scene: after the reserve
        self.counts = 0                                          # bytes of the count planes' fields, which the next edit drops
        self.lab = None                                          # (clipped bounds, labels) of the latest vrt_scene_components step
        self.metal = False
        self.vol = vol
        self.slots = None
        if bricks:
            K = vrt._capi
            self.nb = tuple(d // 8 for d in self.dims)
            ptr = S.device_pointers(self.sc.debug_state(K.STATE_BENTRY), self.nb)
            assert ((ptr != 0) == bc.brick_occupancy(vol)).all()
            self.slots = S.Slots({(int(x), int(y), int(z)): int(ptr[z, y, x]) - 1 for z, y, x in np.argwhere(ptr)}, self.sc.debug_state(K.STATE_BPOOL).shape[0])
            assert len(self.slots.free) == bc.BRICK_SPARE

    def snapshot(self):
        return bc.snapshot(self.vrt, self.sc, self.bricks)

    def held(self):
        """vrt_scene_memory without a dense scene's cell list, whose length is the volume's business (a brick scene's has the
        pool's fixed room)"""
        m = self.sc.memory_bytes()
        return m if self.bricks else m - 4 * self.sc.debug_state(self.vrt._capi.STATE_CELLS).size

    def stale(self, message):
        with pytest.raises(self.vrt._capi.VrtError) as err:
            self.sc.labels()
        assert err.value.code == 1 and message in str(err.value), (self.what, str(err.value))

    def memory(self, allow=0):
        m = self.held()
        assert m >= self.last - allow, (self.what, "vrt_scene_memory fell", self.last, m, allow)
        self.last = m
        return m

    def rewrite(self, k, s, r, checks):
        what = f"{self.what} step {k} ({s['kind']})"
        still = r["refused"] or r["changed"] == 0
        before = self.snapshot() if checks and still else None
        if r["refused"]:
            with pytest.raises(self.vrt._capi.VrtError) as err:
                S.run(self.sc, s, self.second)
            assert err.value.code == 7 and "vrt_scene_reserve_bricks" in str(err.value), what
        else:
            got = S.run(self.sc, s, self.second)
            assert got == r["res"], (what, got, r["res"])
        self.memory(self.counts if r["touched"] else 0)
        if r["touched"]:
            self.counts = 0
        if self.bricks and r["touched"] and not r["refused"]:
            self.slots.edit(self.vol, r["vol"], *S.edited_box(s, r["res"]), s["tool"], k)
        self.vol = r["vol"]
        self.metal = self.metal or (bool(s.get("metal")) and r["changed"] > 0)
        if not checks:
            return
        assert (bc.whole(self.sc, self.dims) == self.vol).all(), what
        if still:
            assert bc.same_snapshot(before, self.snapshot()), what                  # byte for byte as before, slot assignment included
        if self.bricks:
            ptr = S.device_pointers(self.sc.debug_state(self.vrt._capi.STATE_BENTRY), self.nb)
            assert (ptr == self.slots.pointers(self.nb)).all(), (what, "a brick lies in another slot than the model's stack gives it")
        if self.lab is not None:
            if s["tool"] == "filter":                            # (a filter labels for itself)
                self.lab = None
            elif r["touched"]:
                self.stale(S.STALE)
                self.lab = None
            else:                                                # a call that wrote nothing keeps the labelling
                assert (self.sc.labels(self.lab[0]) == self.lab[1]).all(), what

    def ask(self, k, s, checks):
        what = f"{self.what} step {k} ({s['kind']})"
        t = s["tool"]
        before = self.snapshot() if checks else None
        if t == "memory":
            self.memory()
        elif t == "trim":
            self.sc.trim()
            m = self.held()
            assert m == self.base, (what, m, self.base)
            self.last, self.counts, self.lab = m, 0, None
            if checks:
                self.stale(S.NO_LABELS)
        elif t == "trace_rays":
            starts, dirs = query_rays(np.random.default_rng(s["rays"]), 20, self.dims)
            got = self.sc.trace_rays(starts, dirs, MAX_STEPS)
            if checks:
                exp, _ = oracle_records(self.oracle, self.oracle.OracleScene(self.vol, self.pal), starts, dirs, MAX_STEPS)
                assert planes_differ(got, exp).size == 0, what
        elif t == "pick":
            _, push = bc.frame_setup(self.vrt, self.dims)
            xy = np.array([[bc.RES[0] // 2, bc.RES[1] // 2]], np.int32)
            got = self.sc.pick(push, xy, MAX_STEPS)
            if checks:
                o, d = self.oracle.primary_ray(push, int(xy[0, 0]), int(xy[0, 1]))
                exp, _ = oracle_records(self.oracle, self.oracle.OracleScene(self.vol, self.pal), o[None, :], d[None, :], MAX_STEPS)
                assert planes_differ(got, exp).size == 0, what
        else:
            got = S.ask(self.sc, s)
            exp = S.read_expected(self.vol, s) if checks else None
            if checks:
                assert S.same_answer(s, got, exp), (what, got, exp)
            if t == "components" and checks:
                cl, labels = exp[3], exp[2]
                assert (self.sc.labels(cl) == labels).all(), what
                self.lab = (cl, labels)
            elif t == "filter_measure":                          # (a measuring filter labels too, in its own bounds)
                self.lab = None
        if t != "trim":
            self.memory()
        if checks:
            assert bc.same_snapshot(before, self.snapshot()), what

    def check_point(self, k):
        what = f"{self.what} check point after step {k}"
        vrt, engine = self.vrt, self.engine
        bc.assert_state_equals_fresh(vrt, engine, self.sc, self.vol, self.pal, self.bricks, what)
        m0 = self.held()
        exp = bc.assert_frame_equals_oracle(vrt, self.oracle, engine, self.sc, self.vol, self.pal, self.sky, self.noise, self.dims, what, NAMES)
        if self.metal:
            assert (exp["hit_id"] == bc.METAL_ID).any() and int(exp["rays_total"].max()) > 6, what      # the metal is seen, and bounces
        # the count planes' fields were dropped by the edits and built again: the planes equal a fresh scene's
        st, push = bc.frame_setup(vrt, self.dims)
        fresh = bc.make_scene(vrt, engine, self.vol, self.pal, self.bricks, sky=self.sky, noise=self.noise, spare=None)
        got = vrt.GeometryStage(engine, st, self.sc, debug_planes=True).record(push).numpy()
        new = vrt.GeometryStage(engine, st, fresh, debug_planes=True).record(push).numpy()
        engine.synchronize()
        bad = compare_planes(got, new, COUNT_PLANES)
        fresh.destroy()
        assert not bad, (what, bad)
        m1 = self.memory()
        self.counts += m1 - m0

    def play(self, steps, recs, checks=True):
        for k, (s, r) in enumerate(zip(steps, recs)):
            if s["tool"] in S.REWRITING:
                self.rewrite(k, s, r, checks)
            else:
                self.ask(k, s, checks)
            if checks and (k % S.CHECK_EVERY == S.CHECK_EVERY - 1 or k == len(steps) - 1):
                self.check_point(k)
        return self.snapshot()

    def destroy(self):
        self.sc.destroy(); self.second.destroy()


@pytest.mark.parametrize("name,seed", S.TABLE, ids=[f"{n}-seed{s}" for n, s in S.TABLE])
def test_session(vrt, oracle, engine, name, seed):
    dims, bricks = S.VOLUMES[name]
    steps, recs, _ = S.table_model(name, seed)
    first = Player(vrt, oracle, engine, S.start_volume(name), bricks, f"{name} seed {seed}")
    end = first.play(steps, recs)
    assert first.metal and first.held() >= first.base
    first.destroy()
    # from scratch again, the calls alone: the same bytes in every structure, on bricks in the same pool slots
    again = Player(vrt, oracle, engine, S.start_volume(name), bricks, f"{name} seed {seed}, again")
    end2 = again.play(steps, recs, checks=False)
    again.destroy()
    assert same_end(end, end2, bricks), (name, seed, "the second run ends in other bytes")


@pytest.mark.parametrize("kind", sc_.KINDS)
def test_session_on_the_three_streams(vrt, oracle, kind):
    """the short session -- every tool once, then the composed tools again in small bounds -- on the HIP null stream, the context's
    own stream and a side stream of the caller, enqueued behind a stall with no synchronise by the caller in between"""
    import torch
    name = "dense-a"
    dims, bricks = S.VOLUMES[name]
    steps = S.short_session(dims, bricks, 2)
    vol = S.start_volume(name)
    recs, _ = S.run_model(steps, vol, bricks, S.second_volume())
    side = torch.cuda.Stream() if kind == "side" else None
    with torch.cuda.stream(side if side is not None else torch.cuda.default_stream()):
        engine = vrt.Engine(0, use_torch_stream=kind != "own")
        lib, cap = vrt.lib(), vrt._capi
        p = Player(vrt, oracle, engine, vol, bricks, f"stream {kind}", textures=False)
        stall_t, stall_p = None, C.c_void_p()
        if kind == "own":
            cap.check(lib.vrt_device_alloc(engine.ctx, sc_.STALL_BYTES, C.byref(stall_p)))
        else:
            stall_t = torch.zeros(sc_.STALL_BYTES // 4, dtype=torch.float32, device=engine.torch_device)
        torch.cuda.synchronize()
        for k in range(sc_.STALL_PASSES):                                 # the stall
            if kind == "own":
                cap.check(lib.vrt_memset(engine.ctx, stall_p, k, sc_.STALL_BYTES))
            else:
                stall_t.add_(1.0)
        got = []
        for s in steps:
            got.append(S.run(p.sc, s, p.second) if s["tool"] in S.REWRITING else p.sc.trim() if s["tool"] == "trim" else S.ask(p.sc, s))
        read = p.sc.read((0, 0, 0), dims)
        engine.synchronize()
        if kind == "own":
            torch.cuda.synchronize()
            lib.vrt_device_free(engine.ctx, stall_p)
        v = vol
        for k, (s, r, g) in enumerate(zip(steps, recs, got)):
            if s["tool"] in S.REWRITING:
                assert not r["refused"] and g == r["res"], (kind, k, s["kind"], g, r["res"])
            elif s["tool"] != "trim":
                assert S.same_answer(s, g, S.read_expected(v, s)), (kind, k, s["kind"])
            v = r["vol"]
        assert (read == v).all(), kind
        bc.assert_state_equals_fresh(vrt, engine, p.sc, v, p.pal, bricks, f"stream {kind}")
        p.destroy(); engine.destroy()


def test_two_scenes_interleaved(vrt, oracle, engine):
    """a dense scene and a reserved brick scene of one volume on one context, the short session on each with the calls alternating:
    each ends exactly as when run alone (the scratch is the scene's, the brush record the context's: neither leaks)"""
    dims = bc.BRICKS
    vol = bc.brick_volume(dims, 7)
    steps = S.short_session(dims, True, 8)
    recs, _ = S.run_model(steps, vol, True, S.second_volume())
    assert not any(r["refused"] for r in recs)
    alone = {}
    for bricks in (False, True):
        p = Player(vrt, oracle, engine, vol, bricks, f"alone, bricks {bricks}", textures=False)
        alone[bricks] = p.play(steps, recs, checks=False)
        assert (bc.whole(p.sc, dims) == recs[-1]["vol"]).all()
        p.destroy()
    pair = {bricks: Player(vrt, oracle, engine, vol, bricks, f"interleaved, bricks {bricks}", textures=False) for bricks in (False, True)}
    for k, (s, r) in enumerate(zip(steps, recs)):
        for bricks in ((False, True) if k % 2 == 0 else (True, False)):
            p = pair[bricks]
            if s["tool"] in S.REWRITING:
                p.rewrite(k, s, r, True)
            else:
                p.ask(k, s, True)
    for bricks, p in pair.items():
        assert (bc.whole(p.sc, dims) == recs[-1]["vol"]).all(), bricks
        bc.assert_state_equals_fresh(vrt, engine, p.sc, recs[-1]["vol"], p.pal, bricks, f"interleaved, bricks {bricks}")
        assert same_end(alone[bricks], p.snapshot(), bricks), (bricks, "not as when run alone")
        p.destroy()
