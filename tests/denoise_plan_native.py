"""Host build of csrc/vrt_denoise_plan.h (tests/native/denoise_plan_host.cpp): which kernel a denoiser pass takes and the shape of its
launch, asked of the code that launch_denoise_pass runs; the plan's input computed from denoiser settings the way vrt_denoise computes
it; and the stand-alone program of the plan's sweeps under the sanitizers (CPU only; a program of its own, nothing is preloaded)."""
import ctypes as C
import os
import subprocess

import numpy as np

import denoise_shard_common as dsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "denoise_plan_host.cpp")
LIB = os.path.join(ROOT, "tests", "native", "libdenoise_plan_host.so")
HDRS = [os.path.join(ROOT, "voxel-raytracing_amd", "csrc", "vrt_denoise_plan.h"), os.path.join(ROOT, "include", "vrt.h")]

FAMILIES = ("k_denoise", "k_denoise_lds", "k_denoise_fast", "k_denoise_ver", "k_denoise_pair", "k_denoise_p0")      # DenoiseFamily
DENOISE_FAST = 2                                    # VRT_DENOISE_FAST
GUARD_MAX = 0.02                                    # kDenGuardMax (csrc/vrt_denoise_bound.h)
BLOCKS = 3                                          # of denoise_plan_block_c


class PlanIn(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("W", "H")] + [("step_width", C.c_float)] + \
               [(n, C.c_int32) for n in ("phi_inf", "mode", "verified", "packed_ok", "extend", "tile16", "no_packed", "no_pair", "no_p0", "pair_wgs",
                                         "nranks", "strip_rows", "n_local_strips")]


class Plan(C.Structure):
    _fields_ = [("family", C.c_int32), ("key", C.c_uint32)] + \
               [(n, C.c_int32) for n in ("PHI_INF", "SHIPPED", "FAST", "PACKED", "FLAG", "RT", "PASS0", "TH", "pair_R")] + \
               [(n, C.c_uint32) for n in ("grid_x", "grid_y", "block")] + [("lds_bytes", C.c_uint64)] + \
               [(n, C.c_int32) for n in ("R", "seg_rows", "segs")]

    @property
    def name(self):
        return FAMILIES[self.family]

    @property
    def instantiation(self):
        """(family, template arguments in the template's order): one arm of launch_denoise_pass' switch"""
        args = {"k_denoise": ("PHI_INF",), "k_denoise_lds": ("PHI_INF", "SHIPPED", "FAST", "PACKED"), "k_denoise_fast": ("SHIPPED", "TH"),
                "k_denoise_ver": ("SHIPPED", "FLAG", "RT", "PASS0"), "k_denoise_pair": ("FLAG", "pair_R"), "k_denoise_p0": ("FLAG",)}[self.name]
        return (self.name,) + tuple(int(getattr(self, a)) for a in args)


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB) or any(os.path.getmtime(LIB) < os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", LIB, SRC])
    l = C.CDLL(LIB)
    l.denoise_plan_c.argtypes = [C.POINTER(PlanIn), C.POINTER(Plan)]
    l.denoise_plan_c.restype = None
    l.denoise_key_c.argtypes = [C.c_int32] * 5
    l.denoise_key_c.restype = C.c_uint32
    l.denoise_plan_sizes_c.restype = C.c_uint32
    l.denoise_plan_block_c.argtypes = [C.c_int32, C.POINTER(C.c_uint64)]
    l.denoise_plan_block_c.restype = C.c_uint64
    assert l.denoise_plan_sizes_c() == C.sizeof(PlanIn) << 16 | C.sizeof(Plan)
    _lib = l
    return l


def plan(W, H, step_width, phi_inf, mode=0, verified=1, packed_ok=1, extend=0, nranks=1, strip_rows=None, n_local_strips=1, **switches):
    """denoise_plan of one pass.  switches: tile16, no_packed, no_pair, no_p0, pair_wgs."""
    i = PlanIn(W=W, H=H, step_width=step_width, phi_inf=int(phi_inf), mode=mode, verified=int(verified), packed_ok=int(packed_ok), extend=extend,
               nranks=nranks, strip_rows=(H + 15) // 16 * 16 if strip_rows is None else strip_rows, n_local_strips=n_local_strips, **switches)
    q = Plan()
    lib().denoise_plan_c(C.byref(i), C.byref(q))
    assert q.key == lib().denoise_key_c(q.family, *(q.instantiation[1:] + (0,) * 4)[:4])
    return q


def guard(vrt, iterations, step, mode, phis, p):
    ds = vrt._capi.DenoiserSettings()
    vrt.lib().vrt_denoiser_settings_default(C.byref(ds))
    ds.iterations, ds.step_width, ds.mode = iterations, step, mode
    if phis is not None:
        ds.phi_color0, ds.phi_normal0, ds.phi_pos0 = phis
    g = C.c_float()
    vrt._capi.check(vrt.lib().vrt_denoise_guard(C.byref(ds), p, C.byref(g)))
    return float(g.value)


def passes(vrt, W, H, iterations, step, mode=0, phis=None, options=None, shard=None):
    """[Plan] of the passes of one vrt_denoise call, the input of each computed the way vrt_denoise computes it (csrc/vrt_api_post.hip):
    options: the context options of the call ("denoise_verified", "denoise_pair", "denoise_p0", "denoise_packed", "denoise_th16",
    "denoise_pair_wgs"); shard: (rank, nranks, strip_rows) or None.  A rank without a strip launches nothing: []."""
    o = dict(options or {})
    rank, nranks, strip_rows = shard if shard is not None else (0, 1, (H + 15) // 16 * 16)      # (make_shard: one rank is one strip)
    n_local = len(dsc.strips(H, rank, nranks, strip_rows))
    if n_local == 0:
        return []
    f32 = np.float32
    reach = dsc.reaches(iterations, step)
    ph = [f32(v) for v in (dsc.DEFAULT_PHIS if phis is None else phis)]
    out = []
    for i in range(iterations):
        with np.errstate(divide="ignore"):
            inv = f32(1.0) / f32(i)
        phi = [inv * v for v in ph]
        sw = f32(i) * f32(step) + f32(1.0)
        sw2 = sw * sw
        packed_ok = all(f32(2.0) ** -20 <= v <= f32(2.0) ** 20 for v in phi + [sw2])
        verified = bool(o.get("denoise_verified", 1)) and W * H < 1 << 28 and guard(vrt, iterations, step, mode, phis, i) <= GUARD_MAX
        out.append(plan(W, H, float(sw), all(np.isinf(v) for v in phi), mode, verified, packed_ok, sum(reach[i + 1:]) if nranks > 1 else 0,
                        nranks, strip_rows, n_local, tile16=int(o.get("denoise_th16", 0)), no_packed=int(not o.get("denoise_packed", 1)),
                        no_pair=int(not o.get("denoise_pair", 1)), no_p0=int(not o.get("denoise_p0", 1)), pair_wgs=int(o.get("denoise_pair_wgs", 0))))
    return out


def run_main_program(exe):
    """builds the sanitized stand-alone program as `exe` and runs it -> [(block, plans, checksum)]"""
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DDENOISE_PLAN_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-3000:])
    return [tuple(int(w) for w in line.split()) for line in p.stdout.splitlines()]
