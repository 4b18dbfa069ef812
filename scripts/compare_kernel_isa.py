#!/usr/bin/env python3
"""Do two builds of libpom_batch.so hold the same kernels, instruction for instruction?

    python scripts/compare_kernel_isa.py OLD.so NEW.so

Extracts the gfx950 code objects of each library — one per translation unit it was linked from — (llvm-objcopy of .hip_fatbin, one
clang-offload-bundler run per bundle), disassembles them (llvm-objdump -d) and compares, for every kernel symbol that exists in both
libraries, whichever unit holds it, the instruction stream: mnemonics and operands in order, up to the symbol's
size (the padding behind a kernel's last instruction is not part of it).  Left out of the comparison is what only says WHERE the
kernel lies: the addresses and encodings objdump prints beside the instructions, and the 32-bit literal of the s_add_u32 that follows
an s_getpc_b64 — the distance from the kernel to a constant table, which moves when code is added to the library.  Prints one line
per kernel that differs and a summary line; exit status 1 if a common kernel differs.  No GPU needed.

The reason to care: what else a translation unit holds reaches the code of its kernels (the order kernels are emitted in:
pom_issue.h step_kernel; the value ranges of shared bodies' arguments: pom_step_mixed.h).  Units do not reach each other, so a new
kernel family in a unit of its own needs no such proof; a pull request that touches the core unit (pom_batch.hip) shows with this
that it left the headline kernels alone."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("POM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def _run(*cmd) -> str:
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib: str, tmp: str) -> list:
    """the library's gfx950 code objects as files: .hip_fatbin holds one offload bundle per translation unit, each padded to a page"""
    stem = os.path.join(tmp, f"{len(os.listdir(tmp))}")
    _run(os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, stem + ".fatbin")
    blob = open(stem + ".fatbin", "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), blob)]
    assert starts, f"{lib}: no offload bundle in .hip_fatbin"
    out = []
    for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(blob)])):
        fat, co = f"{stem}.{i}.fatbin", f"{stem}.{i}.co"
        with open(fat, "wb") as f:
            f.write(blob[a:b])
        bundler = [os.path.join(LLVM, "clang-offload-bundler"), "--type=o", f"--input={fat}"]
        targets = [t for t in _run(*bundler, "--list").split() if "gfx950" in t]
        assert len(targets) == 1, f"{lib}: gfx950 code objects of bundle {i}: {targets}"
        _run(*bundler, "--unbundle", f"--targets={targets[0]}", f"--output={co}")
        out.append(co)
    return out


def kernels(lib: str, tmp: str) -> dict:
    """{symbol: [instruction text]} of all the library's gfx950 code objects"""
    out = {}
    for co in code_objects(lib, tmp):
        found = kernels_of(co)
        assert not set(found) & set(out), f"{lib}: defined in two units: {sorted(set(found) & set(out))}"
        out.update(found)
    return out


def kernels_of(co: str) -> dict:
    size = {}
    for line in _run(os.path.join(LLVM, "llvm-readelf"), "-s", "--wide", co).splitlines():
        f = line.split()
        if len(f) >= 8 and f[3] == "FUNC":
            size[f[7]] = int(f[2])
    out, name, end, after_getpc = {}, None, 0, False
    for line in _run(os.path.join(LLVM, "llvm-objdump"), "-d", co).splitlines():
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:$", line)
        if m:
            name, end = m.group(2), int(m.group(1), 16) + size.get(m.group(2), 0)
            out[name] = []
            continue
        m = re.match(r"^\s+(.*?)\s*// ([0-9A-Fa-f]+):", line)
        if name is None or not m or int(m.group(2), 16) >= end:
            continue
        ins = re.sub(r"\b[0-9a-f]+ (<[^>]+>)", r"\1", m.group(1))   # a branch target keeps its <symbol+offset>, not its address
        if after_getpc and ins.startswith("s_add_u32"):
            ins = re.sub(r"0x[0-9a-f]+$", "<distance>", ins)
        after_getpc = ins.startswith("s_getpc_b64")
        out[name].append(ins)
    return out


def main() -> int:
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(sys.argv[1], tmp), kernels(sys.argv[2], tmp)
    common = sorted(set(old) & set(new))
    differ = [k for k in common if old[k] != new[k]]
    for k in differ:
        print(f"DIFFERS: {k} ({len(old[k])} -> {len(new[k])} instructions)")
    print(f"{len(common)} kernels in both ({sum(len(old[k]) for k in common)} instructions), {len(differ)} differ; "
          f"only in the old one: {len(set(old) - set(new))}, only in the new one: {len(set(new) - set(old))}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
