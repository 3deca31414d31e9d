"""The product's own .vox reader (csrc/vox_reader.cpp, via the host-only C-ABI entry vrt_vox_flatten_host)
against (a) the committed golden fixtures produced by the reference's ogt_vox.h and (b) the reference parser's results on
generated scenes (recorded; re-derived from the reference parser itself when oracle/_ref is present)."""
import glob
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = sorted(os.path.basename(p)[4:-4] for p in glob.glob(os.path.join(GOLD, "vox_*.vox")))


def test_fixture_inventory():
    assert {"single", "multi", "groups", "raw_default_palette", "raw_imap_matl", "err_no_instance",
            "err_bad_magic", "err_version", "raw_graph_empty_model"} <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_reader_matches_golden(vrt, name):
    data = open(os.path.join(GOLD, f"vox_{name}.vox"), "rb").read()
    exp = np.load(os.path.join(GOLD, f"vox_{name}.npz"))
    rc = int(exp["rc"])
    if rc != 0:
        # reference: throws std::runtime_error (voxel_scene.cpp:46,50)
        with pytest.raises(RuntimeError) as ei:
            vrt.vox_flatten_host(data)
        want = "Could not parse voxel scene" if rc == 1 else "Voxel scene does not contain an instance."
        assert want in str(ei.value)
        return
    vox, pal, ninst, dropped = vrt.vox_flatten_host(data)
    assert vox.shape == exp["voxels"].shape
    assert (vox == exp["voxels"]).all()
    assert ninst == int(exp["ninst"]) and dropped == int(exp["dropped"])
    assert np.allclose(pal, exp["palette"], rtol=1e-6, atol=0)      # powf on the same libm: equal in practice


def test_reader_matches_reference_parser_live(vrt, oracle):
    """25 generated scenes (make_vox_fixtures.live_case_inputs) written by the reference's ogt_vox_write_scene: the product's
    reader against what the reference parser made of them, recorded in refvox_live_cases.npz; where oracle/_ref is present the
    scenes are also written and parsed again by the reference itself and must match the record."""
    import sys
    sys.path.insert(0, GOLD)
    from make_vox_fixtures import LIVE_CASES, live_case_inputs
    rec = np.load(os.path.join(GOLD, "refvox_live_cases.npz"))
    assert int(rec["n"]) == LIVE_CASES
    live = oracle.refvox() is not None
    for case, inputs in enumerate(live_case_inputs()):
        data = rec[f"data{case}"].tobytes()
        evox, epal = rec[f"voxels{case}"], rec[f"palette{case}"]
        eninst, edrop = int(rec[f"ninst{case}"]), int(rec[f"dropped{case}"])
        if live:
            assert oracle.refvox_write(*inputs) == data, f"case {case}"
            rc, lvox, lpal, lninst, ldrop = oracle.refvox_flatten(data)
            assert rc == 0
            assert lvox.shape == evox.shape and (lvox == evox).all() and (lpal == epal).all(), f"case {case}"
            assert lninst == eninst and ldrop == edrop
        vox, gpal, ninst, dropped = vrt.vox_flatten_host(data)
        assert vox.shape == evox.shape and (vox == evox).all(), f"case {case}"
        assert ninst == eninst and dropped == edrop
        assert np.allclose(gpal, epal, rtol=1e-6, atol=0)


def test_truncated_and_garbage_inputs_do_not_crash(vrt):
    data = open(os.path.join(GOLD, "vox_multi.vox"), "rb").read()
    rng = np.random.default_rng(4)
    for cut in list(range(0, 64)) + [len(data) // 2, len(data) - 1]:
        try:
            vrt.vox_flatten_host(data[:cut] if cut else b"\x00")
        except (RuntimeError, vrt.VrtError):
            pass
    for _ in range(50):
        b = bytearray(data)
        for _ in range(8):
            b[int(rng.integers(8, len(b)))] = int(rng.integers(0, 256))
        try:
            vrt.vox_flatten_host(bytes(b))
        except (RuntimeError, vrt.VrtError):
            pass
