"""The argument errors of the three temporal passes -- vrt_reproject, vrt_reproject_camera, vrt_upsample -- as one table of broken
calls, every row applied to each entry point with that function's own argument list, and answered before a context or a device
is looked at (there is none here: a non-NULL fake context, host memory standing for device memory, never dereferenced).

The expected (return code, vrt_last_error() text) pairs are tests/golden/temporal_errors.json, the project's own recorded output:

    VRT_LIB=<a build of libvrt_hip.so> python tests/test_temporal_errors_cpu.py --record

It was recorded on the commit before the three entry points came to share their checks and is not regenerated: the test asserts
code and text verbatim, so the order in which the rules are reported and every word of every message stay what they were."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "temporal_errors.json")
FUNCTIONS = ("vrt_reproject", "vrt_reproject_camera", "vrt_upsample")
PERSPECTIVE, ORTHOGRAPHIC, PANORAMA = 0, 1, 2
GAP = 64            # bytes between two planes: a pointer moved by a few bytes leaves its alignment class and overlaps nothing


class World:
    """One entry point with a complete, valid argument list over fake memory; call(**kw) replaces arguments by name.  The frame is
    w x h texels, the history tw x th (the same but for vrt_upsample).  `W`, `H` name the size the frame-size rules are about:
    the display size of vrt_upsample, the frame size of the other two."""

    def __init__(self, vrt, name):
        self.vrt, self.cap, self.lib, self.name = vrt, vrt._capi, vrt.lib(), name
        cap = self.cap
        self.w, self.h = 48, 32
        self.tw, self.th = (96, 64) if name == "vrt_upsample" else (self.w, self.h)
        n, tn = self.w * self.h, self.tw * self.th
        self.n, self.tn = n, tn
        sizes = dict(col=4 * n, pos=16 * n, nrm=4 * n, hin_c=8 * tn, hin_s=16 * tn, hout_c=8 * tn, hout_s=16 * tn, res=4 * tn, mot=8 * tn)
        self._buf = (C.c_uint8 * (sum(sizes.values()) + GAP * (len(sizes) + 2)))()
        o = (C.addressof(self._buf) + GAP - 1) & ~(GAP - 1)
        at = {}
        for k, v in sizes.items():
            at[k] = o
            o += v + GAP
        self.cur = self.camera()
        st = cap.ReprojectSettings(32, 0.5, 0.1)
        self.base = dict(ctx=C.c_void_p(at["col"]), W=self.tw, H=self.th, cur=self.cur, prev=self.cur, st=st, col=at["col"], pos=at["pos"],
                         nrm=at["nrm"], hin=cap.History(at["hin_c"], at["hin_s"]), hout=cap.History(at["hout_c"], at["hout_s"]),
                         res=at["res"], mot=at["mot"])
        if name == "vrt_upsample":
            self.base.update(w=self.w, h=self.h)
        for k, v in self.base.items():
            setattr(self, k, v)

    def push(self, size=None, **kw):
        v = self.vrt
        ctl = v.CameraController(position=kw.get("pos", (20.3, 20.2, -14.0)), yaw=90.0, pitch=0.0)
        return v.make_push(ctl, (40, 40, 40), size or (self.w, self.h), 1, (0.0, 0.0))

    def camera(self, model=PERSPECTIVE, tan_half=1.0, half_width=10.0, size=None):
        """A valid camera block of this entry point: a push block, or a vrt_ray_camera of `model`."""
        if self.name != "vrt_reproject_camera":
            return self.push(size)
        c = self.cap.RayCamera()
        c.model, c.basis, c.tan_half, c.half_width = model, self.push(size), tan_half, half_width
        return c

    def basis(self, cam):
        return cam.basis if self.name == "vrt_reproject_camera" else cam

    def broken(self, how, **kw):
        """A camera block that is valid but for one thing."""
        c = self.camera(**kw)
        b = self.basis(c)
        if how == "zero_right":
            b.cam_right[:] = [0.0, 0.0, 0.0, 0.0]
        elif how == "inf_up":
            b.cam_up[1] = float("inf")
        elif how == "inf_right":
            b.cam_right[0] = float("inf")
        elif how == "nan_pos":
            b.cam_pos[2] = float("nan")
        elif how == "inf_jitter":
            b.camera_jitter[0] = float("inf")
        else:
            raise KeyError(how)
        return c

    def call(self, **kw):
        a = dict(self.base)
        a.update(kw)
        ref = lambda x: C.byref(x) if x is not None else None
        head = (a["ctx"], a["w"], a["h"], a["W"], a["H"]) if self.name == "vrt_upsample" else (a["ctx"], a["W"], a["H"])
        rc = getattr(self.lib, self.name)(*head, ref(a["cur"]), ref(a["prev"]), ref(a["st"]), a["col"], a["pos"], a["nrm"], ref(a["hin"]),
                                          ref(a["hout"]), a["res"], a["mot"])
        return int(rc), self.lib.vrt_last_error().decode()


def common_rows(x):
    """(row name, replaced arguments) for any of the three entry points; x is its World."""
    H_ = x.cap.History
    S_ = x.cap.ReprojectSettings
    hin, hout = x.hin, x.hout
    nan, inf = float("nan"), float("inf")
    rows = [
        # NULL arguments, the half-NULL vrt_history structs among them
        ("null ctx", dict(ctx=None)), ("null cur", dict(cur=None)), ("null prev", dict(prev=None)), ("null color8", dict(col=None)),
        ("null position", dict(pos=None)), ("null normal8", dict(nrm=None)), ("null history_out", dict(hout=None)),
        ("null history_out.color16", dict(hout=H_(None, hout.surface))), ("null history_out.surface", dict(hout=H_(hout.color16, None))),
        ("null history_in.color16", dict(hin=H_(None, hin.surface))), ("null history_in.surface", dict(hin=H_(hin.color16, None))),
        # frame size
        ("W=0", dict(W=0)), ("H=-1", dict(H=-1)), ("W=40000", dict(W=40000)), ("16384x16384", dict(W=16384, H=16384)),
        # settings
        ("max_history 0", dict(st=S_(0, 0.5, 0.1))), ("max_history 256", dict(st=S_(256, 0.5, 0.1))),
        ("tol_abs negative", dict(st=S_(32, -0.5, 0.1))), ("tol_rel negative", dict(st=S_(32, 0.5, -0.1))),
        ("tol_abs nan", dict(st=S_(32, nan, 0.1))), ("tol_rel nan", dict(st=S_(32, 0.5, nan))),
        ("tol_abs inf", dict(st=S_(32, inf, 0.1))), ("tol_rel inf", dict(st=S_(32, 0.5, inf))),
        # overlap: history out with history in, with an input, with itself, and the optional outputs likewise
        ("overlap history_out is history_in", dict(hout=hin)),
        ("overlap out.color16 is in.color16", dict(hout=H_(hin.color16, hout.surface))),
        ("overlap out.surface is position", dict(hout=H_(hout.color16, x.pos))),
        ("overlap out.surface is out.color16", dict(hout=H_(hout.color16, hout.color16))),
        ("overlap out.color16 inside color8", dict(hout=H_(x.col + 16, hout.surface))),
        ("overlap resolved8 is color8", dict(res=x.col)),
        ("overlap resolved8 inside out.surface", dict(res=hout.surface + 64)),
        ("overlap motion is in.surface", dict(mot=hin.surface)),
        ("overlap motion is resolved8", dict(mot=x.res)),
        ("overlap resolved8 on the last texel of normal8", dict(res=x.nrm + 4 * x.n - 4)),
        ("overlap resolved8 on the last texel of out.color16", dict(res=hout.color16 + 8 * x.tn - 4)),
        ("overlap motion on the last texel of resolved8", dict(mot=x.res + 4 * x.tn - 8)),
        # alignment
        ("misaligned position", dict(pos=x.pos + 4)), ("misaligned motion", dict(mot=x.mot + 4)),
        ("misaligned history_out.color16", dict(hout=H_(hout.color16 + 4, hout.surface))), ("misaligned resolved8", dict(res=x.res + 2)),
        ("misaligned history_in.surface", dict(hin=H_(hin.color16, hin.surface + 8))), ("misaligned color8", dict(col=x.col + 1)),
        # the optional arguments left out, then a later rule
        ("no history_in, overlap", dict(hin=None, res=x.col)), ("no motion, misaligned position", dict(mot=None, pos=x.pos + 4)),
        ("no resolved8, overlap", dict(res=None, mot=hout.surface)),
        # default settings (settings NULL), then a later rule -- or a default that is itself refused
        ("default settings, overlap", dict(st=None, hout=hin)),
        ("default settings, misaligned position", dict(st=None, pos=x.pos + 4)),
        ("default settings from a non-finite cam_right", dict(st=None, cur=x.broken("inf_right"))),
        # two rules at once: the order in which they are reported
        ("null color8 and W=0", dict(col=None, W=0)),
        ("W=0 and max_history 0", dict(W=0, st=S_(0, 0.5, 0.1))),
        ("16384x16384 and max_history 0", dict(W=16384, H=16384, st=S_(0, 0.5, 0.1))),
        ("max_history 0 and tol_abs negative", dict(st=S_(0, -0.5, 0.1))),
        ("max_history 256 and overlap", dict(st=S_(256, 0.5, 0.1), hout=hin)),
        ("tol_rel nan and degenerate previous camera", dict(st=S_(32, 0.5, nan), prev=x.broken("zero_right"))),
        ("degenerate previous camera and overlap", dict(prev=x.broken("zero_right"), hout=hin)),
        ("overlap and misaligned position", dict(hout=hin, pos=x.pos + 4)),
        ("overlap and misaligned motion", dict(res=x.col, mot=x.mot + 4)),
        # the previous camera
        ("previous camera: zero cam_right", dict(prev=x.broken("zero_right"))),
        ("previous camera: infinite cam_up", dict(prev=x.broken("inf_up"))),
    ]
    return rows


def own_rows(x):
    """The rows of one entry point alone: its cameras, its size rules."""
    if x.name == "vrt_reproject":
        return [("current camera: zero cam_right (not looked at)", dict(cur=x.broken("zero_right"), hout=x.hin))]
    if x.name == "vrt_upsample":
        other = x.push((x.tw, x.th))
        return [
            ("current camera: zero cam_right", dict(cur=x.broken("zero_right"))),
            ("current camera: infinite cam_up", dict(cur=x.broken("inf_up"))),
            ("both cameras degenerate", dict(cur=x.broken("zero_right"), prev=x.broken("inf_up"))),
            ("w=0", dict(w=0)), ("h=-1", dict(h=-1)),
            ("display narrower than render", dict(W=x.w - 1)), ("display lower than render", dict(H=x.h - 1)),
            ("display smaller than render and 40000 wide", dict(W=40000, H=x.h - 1)),
            ("screen_size of cur is the display size", dict(cur=other)), ("screen_size of prev is the display size", dict(prev=other)),
            ("w is not screen_size", dict(w=x.w + 1)),
            ("screen_size mismatch and max_history 0", dict(cur=other, st=x.cap.ReprojectSettings(0, 0.5, 0.1))),
            ("16384x16384 and screen_size mismatch", dict(W=16384, H=16384, cur=other)),
        ]
    rows = []
    good = {m: x.camera(m) for m in (PERSPECTIVE, ORTHOGRAPHIC, PANORAMA)}
    for a, b in ((PERSPECTIVE, ORTHOGRAPHIC), (PANORAMA, PERSPECTIVE), (ORTHOGRAPHIC, PANORAMA)):
        rows.append((f"models differ: current {a}, previous {b}", dict(cur=good[a], prev=good[b])))
    rows.append(("models differ and overlap", dict(cur=good[PERSPECTIVE], prev=good[PANORAMA], hout=x.hin)))
    rows.append(("models differ and max_history 0", dict(cur=good[PERSPECTIVE], prev=good[PANORAMA], st=x.cap.ReprojectSettings(0, 0.5, 0.1))))
    for m in (3, -1):
        rows.append((f"both cameras of unknown model {m}", dict(cur=x.camera(m), prev=x.camera(m))))
    bad = []
    for v in (0.0, -1.0, float("nan"), float("inf")):
        bad.append((f"perspective tan_half {v}", x.camera(PERSPECTIVE, tan_half=v)))
        bad.append((f"orthographic half_width {v}", x.camera(ORTHOGRAPHIC, half_width=v)))
    for m, mn in ((PERSPECTIVE, "perspective"), (ORTHOGRAPHIC, "orthographic"), (PANORAMA, "panorama")):
        if m != PANORAMA:
            bad.append((f"{mn} zero cam_right", x.broken("zero_right", model=m)))
            bad.append((f"{mn} infinite cam_up", x.broken("inf_up", model=m)))
        bad.append((f"{mn} nan cam_pos", x.broken("nan_pos", model=m)))
    bad.append(("perspective infinite jitter", x.broken("inf_jitter", model=PERSPECTIVE)))
    for what, c in bad:
        rows.append((f"current camera: {what}", dict(cur=c, prev=good[c.model])))
        rows.append((f"previous camera: {what}", dict(cur=good[c.model], prev=c)))
    rows.append(("panorama with a zero cam_right (not looked at), overlap", dict(cur=x.broken("zero_right", model=PANORAMA),
                                                                               prev=x.broken("zero_right", model=PANORAMA), hout=x.hin)))
    return rows


def table(vrt, name):
    """[(row name, (code, message))] of entry point `name` by the loaded library."""
    x = World(vrt, name)
    out = []
    for row, kw in common_rows(x) + own_rows(x):
        out.append((row, x.call(**kw)))
    assert len({r for r, _ in out}) == len(out), "row names are the fixture's keys"
    return out


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_fixture_holds_the_table(vrt):
    """One entry per (function, row), no more and no fewer; every row is an error, none reached the context."""
    g = _golden()
    assert sorted(g) == sorted(FUNCTIONS)
    for name in FUNCTIONS:
        rows = [r for r, _ in table(vrt, name)]
        assert sorted(g[name]) == sorted(rows), name
        for row, e in g[name].items():
            assert e["code"] in (1, 7) and e["message"].startswith(name + ": "), (name, row, e)
    # the common rows are the same rows for all three
    names = [[r for r, _ in common_rows(World(vrt, n))] for n in FUNCTIONS]
    assert names[0] == names[1] == names[2]


def _check(vrt, name):
    g = _golden()[name]
    wrong = [(row, got, (g[row]["code"], g[row]["message"])) for row, got in table(vrt, name) if got != (g[row]["code"], g[row]["message"])]
    assert wrong == [], f"{name}: {len(wrong)} rows differ from the recorded (code, message); the first: {wrong[0]}"


def test_vrt_reproject_errors_verbatim(vrt):
    _check(vrt, "vrt_reproject")


def test_vrt_reproject_camera_errors_verbatim(vrt):
    _check(vrt, "vrt_reproject_camera")


def test_vrt_upsample_errors_verbatim(vrt):
    _check(vrt, "vrt_upsample")


def test_messages_name_their_function_and_differ_only_there(vrt):
    """A common row's message is the same text in all three entry points apart from the name in front -- but where the rule itself
    differs (the cameras; the frame size rule of vrt_upsample holds more)."""
    g = _golden()
    strip = lambda name, row: g[name][row]["message"][len(name):]
    for row, _ in common_rows(World(vrt, "vrt_reproject")):
        if "camera" in row or "cam_right" in row:
            continue
        texts = {strip(n, row) for n in FUNCTIONS}
        codes = {g[n][row]["code"] for n in FUNCTIONS}
        assert len(texts) == 1 and len(codes) == 1, (row, texts, codes)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: VRT_LIB=<libvrt_hip.so> python tests/test_temporal_errors_cpu.py --record")
    sys.path.insert(0, ROOT)
    import voxel_raytracing_amd as vrt_
    out = {name: {row: {"code": code, "message": msg} for row, (code, msg) in table(vrt_, name)} for name in FUNCTIONS}
    with open(GOLDEN, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("recorded", sum(len(v) for v in out.values()), "entries from", vrt_._capi.LIB_PATH, "->", GOLDEN)
