#!/usr/bin/env python3
"""glsl2cpp.py IN.frag OUT.inc -- textual rewrite of a fragment shader into text a C++ compiler reads behind glsl_shim.h.

ORACLE-side test infrastructure.  The input is read from the reference tree, the output goes to oracle/_ref/ only (git-ignored,
generated at every build, never committed).  The rewrite does what syntax requires and nothing that changes arithmetic: no
expression is reordered, no operand, index or constant is touched.  The rules, all of them:

  R1  `#version` lines are dropped.
  R2  `layout (...)` qualifiers are dropped.
  R3  `in T name;`, `out T name;` and `uniform T name;` become the global `T name;`.
  R4  An interface block `uniform Block { members } instance;` becomes `struct Block { members } instance;`; a block without an
      instance name becomes its members as globals (as GLSL scopes them).
  R5  An array member `T name[N];` of an interface block becomes `ubo_array<T, N> name;` (glsl_shim.h: a byte buffer read with a
      stride, 0 past its end), so that the driver decides the buffer's layout and length, not the compiler.
  R6  A floating literal without a suffix gets `f`: GLSL's literals are 32-bit floats, C++'s are doubles (`dir * 0.01` has to
      multiply by a float).
  R7  A local declaration whose initialiser names the variable it declares (`bool hit = traceRayHit(hit.pos ...`,
      voxel_volume.frag:219) is renamed with a trailing underscore from its declarator to the end of its block: GLSL brings a name
      into scope after its initialiser, C++ inside it.
  R8  A local `S name;` of a struct type S declared in the shader and without an initialiser becomes `S name{};` (value
      initialisation: every member zero, which is the resolution of the uninitialised RayHitInternal / RayHit).

Swizzles, vector constructors and implicit int -> float vector conversions are the header's business.
"""
import re
import sys

FLOAT_LIT = re.compile(r"(?<![\w.])((?:\d+\.\d*|\.\d+)(?:[eE][+-]?\d+)?|\d+[eE][+-]?\d+)(?![\w.])")


def strip_layout(line):
    """R2: remove `layout ( ... )` with balanced parentheses."""
    while True:
        m = re.search(r"\blayout\s*\(", line)
        if not m:
            return line
        depth, i = 1, m.end()
        while depth and i < len(line):
            depth += {"(": 1, ")": -1}.get(line[i], 0)
            i += 1
        line = line[:m.start()] + line[i:].lstrip()


def rewrite(src):
    lines = src.split("\n")
    out, structs = [], set()
    i = 0
    while i < len(lines):
        line = lines[i]
        i += 1
        if line.lstrip().startswith("#version"):                                  # R1
            continue
        line = strip_layout(line)                                                 # R2
        m = re.match(r"^(\s*)uniform\s+(\w+)\s*(\{?)\s*$", line)
        if m:                                                                     # R4: interface block
            indent, block, brace = m.groups()
            if not brace:
                assert lines[i].strip() == "{", lines[i]
                i += 1
            members = []
            while not lines[i].lstrip().startswith("}"):
                members.append(lines[i])
                i += 1
            inst = re.match(r"^\s*\}\s*(\w*)\s*;\s*$", lines[i]).group(1)
            i += 1
            members = [re.sub(r"^(\s*)(\w+)\s+(\w+)\s*\[\s*(\w+)\s*\]\s*;", r"\1ubo_array<\2, \4> \3;", x) for x in members]   # R5
            if inst:
                out += [f"{indent}struct {block}", f"{indent}{{"] + members + [f"{indent}}} {inst};"]
            else:
                out += [re.sub(r"^\s+", indent, x) for x in members]
            continue
        line = re.sub(r"^(\s*)(?:in|out|uniform)\s+(\w+\s+\w+\s*;)", r"\1\2", line)   # R3
        m = re.match(r"^\s*struct\s+(\w+)", line)
        if m:
            structs.add(m.group(1))
        out.append(line)

    # R7 and R8 work on function bodies: track the brace depth.
    res, depth, renames = [], 0, []                # renames: (name, depth at which the declaration stands)
    for line in out:
        code = line.split("//")[0]
        for name, _ in renames:
            line = re.sub(rf"\b{name}\b(?!_)", name + "_", line)
        m = re.match(r"^(\s*)(\w+)\s+(\w+)\s*=\s*(.*);\s*$", code)
        if depth > 0 and m and re.search(rf"\b{m.group(3)}\b", m.group(4)) and m.group(2) != "return":      # R7
            indent, typ, name, init = m.groups()
            line = f"{indent}{typ} {name}_ = {init};"
            renames.append((name, depth))
        m = re.match(r"^(\s*)(\w+)\s+(\w+)\s*;\s*$", code)
        if depth > 0 and m and m.group(2) in structs:                             # R8
            line = f"{m.group(1)}{m.group(2)} {m.group(3)}{{}};"
        depth += code.count("{") - code.count("}")
        renames = [(n, d) for n, d in renames if d <= depth]
        res.append(line)
    text = "\n".join(res)
    text = FLOAT_LIT.sub(lambda m: m.group(1) + "f", text)                        # R6
    return text


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        src = f.read()
    with open(sys.argv[2], "w") as f:
        f.write("// generated by oracle/ref_shader/glsl2cpp.py -- do not commit\n" + rewrite(src))
