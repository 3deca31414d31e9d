#!/usr/bin/env python3
"""Writes tests/golden/refshader_*.npz: the inputs of every case of tests/ref_shader_common.py and what the reference's own shaders,
compiled as C++ (oracle/ref_shader/, built by `make -C oracle ref` where the reference tree lies), compute for them.  Only data is
recorded: inputs and raw float outputs, no shader text.  Needs oracle/_ref/libvrt_refshader.so; run from the repository root:

    python tests/golden/make_refshader_fixtures.py

tests/test_ref_shader_cpu.py calls record() too and requires the files to equal what it returns, wherever the library is present."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_shader_common as rc          # noqa: E402
from oracle import oracle                # noqa: E402


def _geometry(osn, push, par):
    out = oracle.refshader_render(osn, push, par)
    return dict(push=rc.push_bytes(push), params=rc.params_vector(par), **{n: out[n] for n in rc.SHADER_PLANES})


def record():
    """name -> dict of arrays, one per fixture file refshader_<name>.npz."""
    files = {}
    vol, pal, sky, noise = rc.scene()
    files["scene"] = dict(voxels=vol, palette=pal, sky=sky, noise=noise, face_voxels=rc.face_scene())
    osn = oracle.OracleScene(vol, pal, sky=sky, noise=noise)
    for name in rc.GEOMETRY_CASES:
        files["geom_" + name] = _geometry(osn, *rc.geometry_case(oracle, name))
    fsn = oracle.OracleScene(rc.face_scene(), pal, sky=sky, noise=noise)
    files["geom_face"] = _geometry(fsn, *rc.face_case(oracle))
    files["geom_axis"] = _geometry(osn, *rc.axis_case(oracle))
    for w, h in rc.DENOISE_SIZES:
        color, normal, position = rc.denoise_inputs(w, h)
        files[f"denoise_{w}x{h}_in"] = dict(color=color, normal=normal, position=position)
        for mode in (0, 1):
            outs, c = {}, color
            for i in range(3):
                outs[f"pass{i}"] = oracle.refshader_denoise_pass(c, normal, position, oracle.denoise_pass_params(i), mode)
                c = oracle.unorm8(outs[f"pass{i}"])                  # the RGBA8 target the next pass samples
            files[f"denoise_{w}x{h}_mode{mode}"] = outs
    codes = [{}, {}]
    for k, (sw, sh, tw, th) in enumerate(rc.BLIT_SIZES):
        out = oracle.refshader_blit(rc.blit_source(sw, sh, th), tw, th)
        codes[k % 2][f"codes_{sw}x{sh}_{tw}x{th}"] = oracle.unorm8(out)
        codes[k % 2][f"sha256_{sw}x{sh}_{tw}x{th}"] = np.frombuffer(hashlib.sha256(out.tobytes()).digest(), np.uint8)
    files["blit_a"], files["blit_b"] = codes
    return files


if __name__ == "__main__":
    assert oracle.refshader() is not None, "oracle/_ref/libvrt_refshader.so is absent: make -C oracle ref (needs the reference tree)"
    for name, arrays in record().items():
        path = os.path.join(HERE, f"refshader_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"{os.path.getsize(path):8d}  {os.path.basename(path)}")
