"""The one place that compiles host code for the tests: the kernels' rule functions built for the CPU (tests/emul/*.cpp), the callers of
the C-ABI (tests/cpp/*.cpp), the oracle's C files where a program links them, and the small programs that look at the public headers.
Plain functions, no fixtures: a module's own fixture calls shared_lib() / program() and keeps its ctypes lines.  The rules: one flag set
(-Wall -Wextra -Werror everywhere); a source is compiled once per process however many modules ask; no file is written under its final
name (the compiler writes <target>.tmp<pid>, which is renamed: a loaded library keeps its mapping, two sessions that share build/ never
see a half-written file); the sanitizers only in stand-alone programs: nothing here gets a sanitized library loaded into python."""
import hashlib
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "build")
INCLUDES = ["-I" + os.path.join(ROOT, p) for p in ("include", "pomcpp_amd/csrc", "oracle", "tests/emul")]
STRICT = ("-Wall", "-Wextra", "-Werror")
CXX_FLAGS = ("-O2", "-std=c++17", *STRICT, "-Wno-unknown-pragmas", "-fPIC")   # (the pragmas are the kernels' `#pragma unroll`)
C_FLAGS = ("-O2", "-std=c11", *STRICT, "-fPIC")
# program(..., link=POM_BATCH): a caller of the C-ABI, linked with the product library where it lies
POM_BATCH = ("-L" + os.path.join(ROOT, "pomcpp_amd"), "-lpom_batch", "-Wl,-rpath," + os.path.join(ROOT, "pomcpp_amd"),
             "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib", "-lamdhip64", "-pthread")
SANITIZE = ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan")

_commands = []   # every argv run in this process, in order
_objects = {}    # digest of a compile line and its source's text -> the object
_linked = {}     # target -> the link line that made what lies there


def commands():
    """the compiler and linker command lines run in this process so far (argv lists; an output is named <target>.tmp<pid>)"""
    return [list(c) for c in _commands]


def _run(argv):
    _commands.append(argv)
    done = subprocess.run(argv, cwd=ROOT, capture_output=True, text=True)
    sys.stderr.write(done.stderr)   # what the compiler said, for the test's report
    done.check_returncode()         # subprocess.CalledProcessError, with .stderr


def _make(argv, target):
    os.makedirs(os.path.dirname(target), exist_ok=True)
    tmp = f"{target}.tmp{os.getpid()}"
    _run([*argv, "-o", tmp])   # (a compiler that fails leaves no output behind)
    os.replace(tmp, target)
    return target


def _object(source, flags):
    """one source (relative to the repository, or absolute) to one object under build/obj, by its language's compiler"""
    source = os.path.join(ROOT, source)
    argv = [*(("gcc", *C_FLAGS) if source.endswith(".c") else ("g++", *CXX_FLAGS)), *flags, *INCLUDES, "-c", source]
    # (the text too: a test may write another program to the same path)
    tag = hashlib.sha1("\0".join(argv).encode() + open(source, "rb").read()).hexdigest()[:12]
    if tag not in _objects:
        _objects[tag] = _make(argv, os.path.join(BUILD, "obj", f"{os.path.basename(source)}.{tag}.o"))
    return _objects[tag]


def _link(kind, sources, name, flags, link):
    sources = [sources] if isinstance(sources, str) else list(sources)
    first = os.path.join(ROOT, sources[0])
    stem = os.path.splitext(os.path.basename(first))[0]
    # under build/; beside the source where a test wrote that to its tmp_path
    target = os.path.join(BUILD if first.startswith(ROOT + os.sep) else os.path.dirname(first), name or ("lib" + stem + ".so" if kind else stem))
    objs = [_object(s, flags) for s in sources]
    argv = ["g++", *kind, *[f for f in flags if f.startswith(("-fsanitize", "-static-lib", "-pthread"))], *objs, *link]
    if _linked.get(target) != argv:
        _make(argv, target)
        _linked[target] = argv
    return target


def shared_lib(sources, name=None, extra=()):
    """build/lib<first source's stem>.so (or build/<name>) from the sources, for ctypes.CDLL; `extra` goes to every compile"""
    if any("-fsanitize" in f for f in extra):
        raise ValueError("a sanitized library cannot be loaded into python: sanitize a stand-alone program (program(..., sanitize=True))")
    return _link(["-shared"], sources, name, tuple(extra), ())


def program(sources, name=None, extra=(), link=(), sanitize=False):
    """build/<first source's stem> (or build/<name>): an executable with its own main, to be run as a child process.  `extra` goes to
    every compile, after the flag set (so a -O1 there holds), `link` to the end of the link line (-L.. -l.. -Wl,..); sanitize=True
    builds it with ASan and UBSan, their runtimes linked in: nothing about how it is started matters to them"""
    return _link([], sources, name, (*extra, *(SANITIZE if sanitize else ())), link)


def syntax_check(text, tmp_path, compiler, std, extra_includes=()):
    """`text` as a C ("gcc") or C++ ("g++") file that includes the public headers: it must compile without a warning"""
    src = tmp_path / ("spec.c" if compiler == "gcc" else "spec.cpp")
    src.write_text(text)
    _run([compiler, std, *STRICT, "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), *["-I" + i for i in extra_includes], str(src)])


def header_constant(name):
    """the value include/pom_batch.h gives the enumerator `name`"""
    return int(re.search(rf"\b{name} = (\d+)", open(os.path.join(ROOT, "include", "pom_batch.h")).read()).group(1))
