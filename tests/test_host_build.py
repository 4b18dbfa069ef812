"""tests/host_build.py keeps its own rules: one compile per process, the strict flags on every compile, no sanitized library, a loaded
library survives its rebuild, and a warning is an error."""
import ctypes as C
import os
import subprocess

import pytest

from tests import host_build

REACH = "tests/emul/pom_reach_emul.cpp"


def test_the_same_library_is_compiled_once():
    first = host_build.shared_lib(REACH)
    before = host_build.commands()
    assert host_build.shared_lib(REACH) == first and host_build.commands() == before
    assert sum("-c" in c and c[-3].endswith(REACH) for c in before) == 1


def test_every_compile_carries_the_strict_flags(tmp_path):
    host_build.shared_lib(REACH)
    (tmp_path / "main.c").write_text("int main(void) { return 0; }\n")
    host_build.program(str(tmp_path / "main.c"))
    host_build.syntax_check('#include "pom_batch.h"\n', tmp_path, "gcc", "-std=c99")
    compiles = [c for c in host_build.commands() if "-c" in c or "-fsyntax-only" in c]
    assert {c[0] for c in compiles} == {"gcc", "g++"}
    for c in compiles:
        assert {"-Wall", "-Wextra", "-Werror"} <= set(c), c
        assert not [f for f in c if f.startswith("-Wno-") and f != "-Wno-unknown-pragmas"], c
        assert "-c" not in c or ("-fPIC" in c and ("-std=c11" if c[0] == "gcc" else "-std=c++17") in c), c


def test_no_sanitized_library():
    for extra in (["-fsanitize=address"], ["-O1", "-fno-sanitize-recover=all", "-fsanitize=undefined"]):
        with pytest.raises(ValueError):
            host_build.shared_lib(REACH, name="libsanitized.so", extra=extra)


def test_a_loaded_library_survives_its_rebuild(tmp_path):
    src = tmp_path / "answer.cpp"
    src.write_text('extern "C" int answer(void) { return ANSWER; }\n')
    path = host_build.shared_lib(str(src), name="libanswer.so", extra=["-DANSWER=41"])
    old, inode = C.CDLL(path), os.stat(path).st_ino
    assert old.answer() == 41
    assert host_build.shared_lib(str(src), name="libanswer.so", extra=["-DANSWER=42"]) == path
    assert os.stat(path).st_ino != inode and old.answer() == 41   # a new file under the name, not the mapped one written over
    copy = tmp_path / "libanswer2.so"                              # (dlopen of the same path would hand back the loaded one)
    copy.write_bytes(open(path, "rb").read())
    assert C.CDLL(str(copy)).answer() == 42                       # and the new file is whole
    assert not [f for f in os.listdir(tmp_path) if ".tmp" in f]


def test_a_warning_fails_the_build(tmp_path):
    src = tmp_path / "unused.cpp"
    src.write_text('extern "C" int f(void)\n{\n    int unused = 3; return 0;\n}\n')
    with pytest.raises(subprocess.CalledProcessError) as e:
        host_build.shared_lib(str(src))
    assert "unused" in e.value.stderr and not os.path.exists(tmp_path / "libunused.so")
