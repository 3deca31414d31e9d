"""The reference of the segment queries (vrt_trace_segments, vrt_occluded_segments; csrc/vrt_query_seg.h): boxIntersection, traceRayInt
and traceRay (voxel_volume.frag:109-196) restated in plain float32 numpy, every operation one rounding in the shader's order, with what
the record of vrt_ray_hits does not hold: the advance t_adv boxIntersection gave the origin, the length d that RayHit.pos is made
with, and the iteration of the hit.  `trace` runs a batch, one ray per array element -- the arithmetic of a ray is the scalar loop's,
rays only share the Python interpreter --, `trace_one` a single ray.

Nothing here is trusted on its own account: tests/test_segments_cpu.py first holds material, pos (bit pattern), voxel, mask and
steps to oracle.trace_ray for every ray it uses (`differs_from_oracle`); only then is t_hit = t_adv + d the expected value, and
`segment_records` the expected output of a segment query."""
import numpy as np

F = np.float32
INT_MAX, INT_MIN = 2147483647, -2147483648


def _floor_to_int(x):
    """ivec3(floor(x)) with the conversion the GPU's instruction performs: saturating, NaN -> 0"""
    f = np.floor(x)
    out = np.zeros(f.shape, np.int64)
    ok = ~np.isnan(f)
    out[ok] = np.clip(f[ok].astype(np.float64), INT_MIN, INT_MAX).astype(np.int64)
    return out


def trace(vol, starts, dirs, max_steps):
    """traceRay of every ray of a batch on the dense volume vol[z, y, x].  Returns a dict of arrays: material (uint32), pos (float32
    [n, 3]; 0 on a miss), voxel (the hit's mapPos; 0 on a miss), mask (bits 0..2 of the final mask; 0 on a miss), steps (voxels
    fetched: a hit in iteration k, counted from 0, has fetched k + 1), t_adv, d and t = t_adv + d (all 0 on a miss)."""
    D, H, W = vol.shape
    s = np.ascontiguousarray(starts, F).reshape(-1, 3)
    dr = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = len(s)
    size = np.array([W, H, D], F)
    with np.errstate(all="ignore"):
        inv = F(1.0) / dr                                                     # :110
        t1 = (-s) * inv                                                      # :112
        t2 = (size[None, :] - s) * inv                                       # :113
        tmn, tmx = np.fmin(t1, t2), np.fmax(t1, t2)                          # :114-115 (min / max that drop a NaN, as the oracle's)
        tmin = np.fmax(tmn[:, 0], np.fmax(tmn[:, 1], tmn[:, 2]))             # :117
        tmax = np.fmin(tmx[:, 0], np.fmin(tmx[:, 1], tmx[:, 2]))             # :118
        moved = (tmin >= F(0.0)) & (tmax >= tmin)                            # :120
        t_adv = np.where(moved, tmin + F(0.1), F(0.0)).astype(F)
        p = np.where(moved[:, None], s + (t_adv[:, None] * dr).astype(F), s).astype(F)      # :121 / :123
        mask = np.where(moved[:, None], tmn == tmin[:, None], False)        # the oracle's rule A: the axes of entry
        mp = _floor_to_int(p)                                                # :135
        delta = np.abs(inv)                                                  # :138
        sg = ((dr > 0).astype(F) - (dr < 0).astype(F))                       # :141 sign()
        step = sg.astype(np.int64)
        side = ((((sg * (mp.astype(F) - p)).astype(F) + (sg * F(0.5)).astype(F)).astype(F) + F(0.5)).astype(F) * delta).astype(F)   # :144
        material = np.zeros(n, np.uint32)
        steps = np.zeros(n, np.uint32)
        live = np.ones(n, bool)
        dims = np.array([W, H, D], np.int64)
        for _ in range(int(max_steps)):                                      # :146
            live &= ((mp >= 0) & (mp < dims[None, :])).all(axis=1)           # :149-154
            if not live.any():
                break
            idx = np.flatnonzero(live)
            m = vol[mp[idx, 2], mp[idx, 1], mp[idx, 0]]                      # :157
            steps[idx] += 1
            material[idx] = m
            live[idx[m != 0]] = False                                        # :158
            idx = idx[m == 0]
            if idx.size == 0:
                break
            sd = side[idx]
            mk = np.stack([sd[:, 0] <= np.fmin(sd[:, 1], sd[:, 2]), sd[:, 1] <= np.fmin(sd[:, 2], sd[:, 0]),
                           sd[:, 2] <= np.fmin(sd[:, 0], sd[:, 1])], axis=1)                                         # :164
            mask[idx] = mk
            side[idx] = np.where(mk, (sd + delta[idx]).astype(F), sd)        # :167
            mp[idx] += np.where(mk, step[idx], 0)                            # :170
        hit = material != 0
        mm = np.where(mask, (side - delta).astype(F), F(0.0)).astype(F)      # :191
        d = np.sqrt((((mm[:, 0] * mm[:, 0]).astype(F) + (mm[:, 1] * mm[:, 1]).astype(F)).astype(F) + (mm[:, 2] * mm[:, 2]).astype(F)).astype(F)).astype(F)
        pos = (p + (d[:, None] * dr).astype(F)).astype(F)                    # :192
        t = (t_adv + d).astype(F)
    z3 = np.zeros((n, 3))
    return {"material": material, "pos": np.where(hit[:, None], pos, z3).astype(F), "voxel": np.where(hit[:, None], mp, 0).astype(np.int32),
            "mask": np.where(hit, (mask * np.array([1, 2, 4])).sum(axis=1), 0).astype(np.uint32), "steps": steps,
            "t_adv": np.where(hit, t_adv, 0).astype(F), "d": np.where(hit, d, 0).astype(F), "t": np.where(hit, t, 0).astype(F),
            "step": step.astype(np.int32)}


def trace_one(vol, start, direction, max_steps):
    """One ray: the values of `trace` as scalars / 3-vectors."""
    r = trace(vol, np.asarray(start, F)[None, :], np.asarray(direction, F)[None, :], max_steps)
    return {k: v[0] for k, v in r.items()}


def oracle_trace(oracle, osn, starts, dirs, max_steps):
    """oracle.trace_ray of every ray as arrays: material, pos, voxel, mask (all 0 on a miss) and steps."""
    n = len(starts)
    out = {"material": np.zeros(n, np.uint32), "pos": np.zeros((n, 3), F), "voxel": np.zeros((n, 3), np.int32),
           "mask": np.zeros(n, np.uint32), "steps": np.zeros(n, np.uint32)}
    for i in range(n):
        h = oracle.trace_ray(osn, starts[i], dirs[i], max_steps)
        out["steps"][i] = h.steps
        if h.material != 0:
            out["material"][i] = h.material; out["pos"][i] = list(h.pos); out["voxel"][i] = list(h.voxel); out["mask"][i] = h.mask
    return out


def differs_from_oracle(ref, orc):
    """Indices of the rays on which `ref` (trace's result) and `orc` (oracle_trace's) differ in material, pos (bit pattern), voxel,
    mask or steps."""
    bad = (ref["material"] != orc["material"]) | (ref["steps"] != orc["steps"]) | (ref["mask"] != orc["mask"])
    bad |= (ref["pos"].view(np.uint32) != orc["pos"].view(np.uint32)).any(axis=1) | (ref["voxel"] != orc["voxel"]).any(axis=1)
    return np.flatnonzero(bad)


def segment_records(ref, t_max):
    """What a segment query returns for the rays of `ref` under the limits t_max: vrt_ray_hits' four planes, "t" and "occluded".  A
    hit is kept iff t <= t_max in float32 (NaN: no)."""
    t_max = np.asarray(t_max, F)
    with np.errstate(invalid="ignore"):
        keep = (ref["material"] != 0) & (ref["t"] <= t_max)
    nrm = np.where(((ref["mask"][:, None] >> np.arange(3)[None, :]) & 1).astype(bool), -ref["step"], 0)
    k3 = keep[:, None]
    return {"material": np.where(keep, ref["material"], 0).astype(np.uint8), "pos": np.where(k3, ref["pos"], 0).astype(F),
            "voxel": np.where(k3, ref["voxel"], 0).astype(np.int32), "normal": np.where(k3, nrm, 0).astype(np.int8),
            "t": np.where(keep, ref["t"], 0).astype(F), "occluded": keep.astype(np.uint8)}
