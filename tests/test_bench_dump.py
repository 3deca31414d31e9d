"""bench.py --dump-outputs without a GPU: dump_outputs() on stand-in G-buffers (CPU tensors) writes every plane as float32,
the same seeded pixels on every call, within the size budget."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(torch, F=5, H=36, W=50):
    g = torch.Generator().manual_seed(3)
    gbs = []
    for _ in range(F):
        planes = {"color8": torch.randint(0, 256, (H, W, 4), dtype=torch.uint8, generator=g),
                  "depth": torch.rand((H, W), generator=g),
                  "normal8": torch.randint(-127, 128, (H, W, 4), dtype=torch.int8, generator=g)}
        gbs.append(types.SimpleNamespace(planes=planes))
    return types.SimpleNamespace(gbs=gbs, H=H, W=W)


def test_dump_outputs_seeded_sample(tmp_path, monkeypatch):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 1000)
    sb = _batch(torch)
    F, H, W = len(sb.gbs), sb.H, sb.W
    bench.dump_outputs(str(tmp_path / "a"), torch, sb, 1, 0)
    bench.dump_outputs(str(tmp_path / "b"), torch, sb, 1, 0)
    assert sorted(os.listdir(tmp_path / "a")) == ["color8.npy", "depth.npy", "normal8.npy"]
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, F * H * W, 1000))
    for n in ("color8", "depth", "normal8"):
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        full = torch.stack([g.planes[n] for g in sb.gbs]).reshape(F * H * W, -1).to(torch.float32).numpy()[idx]
        assert np.array_equal(a, full[:, 0] if full.shape[1] == 1 else full)


def test_dump_budget(vrt):
    """Every plane of the bench's G-buffers at DUMP_SAMPLES pixels stays within 64 MB."""
    sys.path.insert(0, ROOT)
    import bench
    host = sys.modules["voxel_raytracing_amd.host"]
    floats_per_pixel = sum(int(np.prod(host._PLANE_SPECS[n][1])) for n in host.GBUFFER_PLANES)
    assert bench.DUMP_SAMPLES * floats_per_pixel * 4 <= 64 * 2 ** 20
