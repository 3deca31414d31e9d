"""vrt_app --brush ... --save-vox OUT (the C++ mirror's VoxelScene::brush): the saved file loads to the volume numpy composes with
tests/brush_reference.py from the same brushes and fills, applied in command-line order."""
import os
import subprocess

import numpy as np
import pytest

import brush_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = os.path.join(ROOT, "voxel-raytracing_amd", "host", "vrt_app")


def test_brushes_and_fills_in_order_then_save(vrt, tmp_path):
    assert os.path.exists(APP), "build with __graft_entry__.build()"
    path = os.path.join(ROOT, "tests", "golden", "vox_multi.vox")
    vol = vrt.vox_flatten_host(open(path, "rb").read())[0].copy()
    D, H, W = vol.shape
    c = (W // 2, H // 2, D // 2)
    r = max(1.5, min(W, H, D) / 3.0 // 0.5 * 0.5)
    out = tmp_path / "brushed.vox"
    args = ["--brush", f"sphere:set:{c[0] + 0.5},{c[1]},{c[2] + 0.5},{r}:9",
            "--fill", "0", "0", "0", str(min(W, 3)), str(min(H, 2)), "1", "7",
            "--brush", f"box:replace:-2,-2,-2,{W + 4},{H + 4},{D + 4}:11:7",
            "--brush", f"capsule:add:0,0,0,{W},{H},{D},1.5:12",
            "--brush", f"ellipsoid:paint:{c[0]},{c[1] + 0.5},{c[2]},{r},1,1.5:13",
            "--brush", f"sphere:set:{-3 * W},0,0,2:14"]
    p = subprocess.run([APP, "--vox", path] + args + ["--save-vox", str(out)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    h = lambda v: int(round(2 * v))
    vol, r1 = R.brush(vol, R.ELLIPSOID, R.SET, [h(c[0] + 0.5), h(c[1]), h(c[2] + 0.5), h(r), h(r), h(r)], 9)
    vol[0:1, 0:min(H, 2), 0:min(W, 3)] = 7
    vol, _ = R.brush(vol, R.BOX, R.REPLACE, [-2, -2, -2, W + 4, H + 4, D + 4], 11, 7)
    vol, _ = R.brush(vol, R.CAPSULE, R.ADD, [0, 0, 0, h(W), h(H), h(D), 3], 12)
    vol, _ = R.brush(vol, R.ELLIPSOID, R.PAINT, [h(c[0]), h(c[1] + 0.5), h(c[2]), h(r), 2, 3], 13)
    assert r1[0] > 0 and (vol == 11).any() and (vol == 12).any() and (vol == 13).any() and not (vol == 7).any()
    assert f"brush: {r1[0]} voxels changed" in p.stdout and "brush: 0 voxels changed" in p.stdout
    got = vrt.vox_flatten_host(out.read_bytes())[0]
    assert got.shape == vol.shape and (got == vol).all()
    bad = subprocess.run([APP, "--vox", path, "--brush", "sphere:set:1.25,2,2,1:9", "--save-vox", str(out)], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "0.5" in bad.stderr
