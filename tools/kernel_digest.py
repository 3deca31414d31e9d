#!/usr/bin/env python3
"""One line per gfx950 kernel of the given object files: mangled name, a hash of its machine code, its resources.

    python3 tools/kernel_digest.py voxel-raytracing_amd/csrc/*.o > after.txt

A pull request that claims to leave kernels alone shows it by an identical listing before and after.  The hash covers the
instruction encodings in order (the hex words of `llvm-objdump -d`, without the address column: branch operands are relative,
so a kernel that merely moved hashes the same; the padding behind a kernel's last instruction is left out); the resources are those of the code object's notes -- VGPRs, SGPRs, private
(scratch) and group (LDS) segment bytes, kernel argument bytes.  Needs the LLVM tools of ROCm, no GPU."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
NOTES = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size")


def run(tool, *args):
    return subprocess.run([os.path.join(LLVM, tool)] + list(args), check=True, stdout=subprocess.PIPE, text=True).stdout


def kernels_of(obj, tmp):
    """{mangled name: (hash of the code, {note: value})} of the gfx950 code object bundled in a host object"""
    fat, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "co")
    run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat)
    if os.path.getsize(fat) == 0:
        return {}                                                     # a host-only object
    run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co)
    notes = {}
    for entry in re.split(r"\n  - ", run("llvm-readelf", "--notes", co)):   # one entry of amdhsa.kernels each
        f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)$", entry, re.M))
        if "name" in f:
            notes[f["name"]] = f
    code, words = {}, None
    for line in run("llvm-objdump", "-d", co).splitlines():
        m = re.match(r"[0-9a-f]+ <(\S+)>:$", line)
        if m:
            words = code.setdefault(m.group(1), [])
        elif words is not None and "//" in line:
            words.append(" ".join(line.split("//")[-1].split(":", 1)[1].split("<")[0].split()))   # "address: WORD WORD <branch target>"
    for words in code.values():
        while words and words[-1] == "BF800000":                      # s_nop 0 behind the last instruction: the section's padding
            words.pop()
    return {n: (hashlib.sha256("\n".join(code[n]).encode()).hexdigest()[:16], f) for n, f in notes.items()}


if __name__ == "__main__":
    kernels = {}
    with tempfile.TemporaryDirectory() as tmp:
        for obj in sys.argv[1:]:
            for name, k in kernels_of(obj, tmp).items():
                if name in kernels:
                    sys.exit(f"{name}: in more than one object")
                kernels[name] = k
    for name in sorted(kernels):
        h, f = kernels[name]
        print(name, h, *(f"{n}={f[n]}" for n in NOTES))
    print(f"{len(kernels)} kernels", file=sys.stderr)
