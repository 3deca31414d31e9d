"""Each march header (csrc/vrt_march_*.h) and the dispatch over them (csrc/vrt_traverse.h) includes what it uses: a translation
unit that includes only that header is accepted by the host compiler of the unit tests and by hipcc as HIP for gfx950 (the device
pass, where the assembly loops and the pools appear).  Syntax only: nothing is built, nothing runs."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "voxel-raytracing_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HEADERS = ("vrt_march_df.h", "vrt_march_fast.h", "vrt_march_brick.h", "vrt_march_literal.h", "vrt_traverse.h")


def _accepts(cmd, cwd):
    p = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, " ".join(cmd) + "\n" + p.stdout[-3000:]


@pytest.mark.parametrize("header", HEADERS)
def test_header_stands_alone(header, tmp_path):
    line = '#include "%s"\n' % os.path.join(CSRC, header)
    (tmp_path / "alone.cpp").write_text(line)
    (tmp_path / "alone.hip").write_text(line)
    _accepts(["g++", "-std=c++17", "-fsyntax-only", "alone.cpp"], str(tmp_path))
    _accepts([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "alone.hip"], str(tmp_path))
