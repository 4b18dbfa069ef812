#!/usr/bin/env python3
"""scripts/kernel_asm_diff.py A.s B.s — two device assemblies of one unit of the library compared kernel by kernel: one line per kernel with its
lines in each and `identical` or `differs`.  It compares text and looks for no particular instruction.

The inputs (the core unit takes about 2.5 minutes; the units: __graft_entry__.HIP_UNITS), compiled as the library is:
  python -c "import subprocess, __graft_entry__ as ge; subprocess.run(ge.hip_compile_cmd('pom_batch', flags=['--cuda-device-only', '-S', '-o', 'A.s']), check=True)"
A kernel is the text from its label to its .Lfunc_end; comments and the .loc / .file / .cfi lines are dropped.  Local labels and the
numbered temporaries (.LBB12_3, .Ltmp40) carry the function's position in the file, which moves when an earlier function does: they
are renumbered in the order the kernel's text names them."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        if not line or re.match(r"\s*\.(loc|file|cfi_\w+)\b", line):
            continue
        m = re.match(r"\s*\.type\s+(\w+),@function$", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            seen = {}  # .LBB<function>_<block>, .Ltmp<k>: renumbered in the order the kernel's text names them
            text = re.sub(r"\.L(BB\d+_|tmp|func_begin|func_end)\d+", lambda t: seen.setdefault(t.group(0), ".L%d" % len(seen)), "\n".join(body))
            out[name], name = text.split("\n"), None
        elif name:
            body.append(line)
    return out


def main(a_path, b_path):
    a, b = kernels(a_path), kernels(b_path)
    same = 0
    for name in sorted(set(a) | set(b)):
        la, lb = a.get(name), b.get(name)
        verdict = "only in " + (a_path if lb is None else b_path) if la is None or lb is None else "identical" if la == lb else "differs"
        same += verdict == "identical"
        print(f"{name:<82} {len(la or ()):>6} {len(lb or ()):>6}  {verdict}")
    print(f"{len(set(a) | set(b))} kernels, {same} identical")


if __name__ == "__main__":
    main(*sys.argv[1:3])
