"""The C-ABI library builds for gfx950, loads, exports every symbol include/pom_batch.h declares, and
fails loudly (no CPU fallback) where there is no HIP device.  No compute calls here."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests.host_build import ROOT, syntax_check


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "pom_batch.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pom_[a-z_]+)\s*\(", text)))


def test_exports_match_header(hip_lib):
    syms = _declared_symbols()
    assert "pom_batch_step" in syms and "pom_step" in syms and len(syms) >= 18
    for s in syms:
        assert hasattr(hip_lib, s), f"{s} declared in include/pom_batch.h but not exported"


def test_exports_nothing_internal(hip_lib):
    """The library is linked from several translation units that share host functions (pom_host.h): those are hidden.  Every defined
    dynamic symbol is a call of include/pom_batch.h, a kernel (its handle, its launch stub, the compiler's per-unit id), or a weak
    instantiation of the C++ library's templates and the implicit members of the two types they are instantiated over."""
    from pomcpp_amd.batch import library_path
    declared = set(_declared_symbols())
    out = subprocess.run(["nm", "-D", "--defined-only", library_path()], capture_output=True, text=True, check=True).stdout
    syms = [line.split()[1:] for line in out.splitlines()]
    assert len(syms) > len(declared)
    std = re.compile(r"_ZNK?(St|9__gnu_cxx)|_ZT[ISV]NSt")
    internal = []
    for kind, name in syms:
        if kind == "T" and name in declared:
            continue
        if re.fullmatch(r"(_Z\d+)?(__device_stub__)?pom_[a-z_]+_kernel.*", name) or (kind == "B" and name.startswith("__hip_cuid_")):
            continue
        if kind in "WV" and (std.match(name) or name in ("_ZN8PomBatchC2Ev", "_ZN9PomIssuerD2Ev")):
            continue
        internal.append((kind, name))
    assert not internal, internal


def test_library_is_a_gfx950_code_object(hip_lib):
    from pomcpp_amd.batch import library_path
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/clang-offload-bundler", "--list", "--type=o", f"--input={library_path()}"],
                         capture_output=True, text=True)
    blob = open(library_path(), "rb").read()
    assert b"gfx950" in blob, out.stdout


def test_header_compiles_as_c_and_cpp(tmp_path):
    text = '#include "pom_batch.h"\nint main(void){ PomBatchOptions o; o.struct_size = sizeof o; return o.struct_size == 0; }\n'
    for cc, std in (("gcc", "-std=c11"), ("g++", "-std=c++17")):
        syntax_check(text, tmp_path, cc, std)


def test_state_layout_matches_reference_offsets():
    from pomcpp_amd.state import STATE_DTYPE
    f = STATE_DTYPE.fields
    assert STATE_DTYPE.itemsize == 1004
    assert [f[k][1] for k in ("board", "timeStep", "aliveAgents", "agents", "bombs_queue", "bombs_index", "bombs_count",
                              "flames_queue", "flames_index", "flames_count")] == [0, 484, 488, 492, 588, 668, 672, 676, 996, 1000]


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="only meaningful where no GPU is present")
def test_no_cpu_fallback_without_a_gpu(hip_lib):
    from pomcpp_amd.batch import BatchEnvironment, PomError, step_one
    from pomcpp_amd.state import new_states
    with pytest.raises(PomError) as e:
        BatchEnvironment(64)
    assert e.value.code == 2  # POM_E_HIP
    with pytest.raises(PomError):
        step_one(new_states(1), np.zeros(4, dtype=np.int32))


def _fail_another_call(lib):
    """leaves another call's text in pom_last_error"""
    assert lib.pom_batch_create(None, 0, None) == 1 and lib.pom_last_error().decode().startswith("pom_batch_create: ")


def test_every_refusing_call_names_itself(hip_lib):
    """Every call of the header but the three that cannot refuse, made with a NULL handle and zero / NULL for everything else right after
    ANOTHER call has failed: POM_E_ARG, and pom_last_error() names the call that refused, not the one before it.  No device needed."""
    lib = hip_lib
    syms = [s for s in _declared_symbols() if s not in ("pom_last_error", "pom_device_count", "pom_batch_size")]
    assert len(syms) >= 52
    wrong = []
    for s in syms:
        fn = getattr(lib, s)
        assert fn.argtypes, f"{s}: pomcpp_amd.batch.load_library declares no argument types for it"
        args = [0 if t in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64) else None for t in fn.argtypes]
        _fail_another_call(lib)
        if s == "pom_batch_create":   # (the other call must be another one)
            assert lib.pom_batch_destroy(None) == 1 and lib.pom_last_error().decode().startswith("pom_batch_destroy: ")
        rc, text = fn(*args), lib.pom_last_error().decode()
        if rc != 1 or not text.startswith(s + ": "):
            wrong.append((s, rc, text))
    assert not wrong, f"{len(wrong)} of {len(syms)}:\n" + "\n".join(map(str, wrong))


def test_one_error_text_across_the_library_s_units(hip_lib):
    """pom_last_error reads ONE text, whichever translation unit wrote it: a call of the core unit fails, then a call of a kernel
    family's unit, then one of the core again — each time the text is the last call's"""
    lib = hip_lib
    _fail_another_call(lib)                                                     # pom_batch.hip
    for family in ("pom_batch_forecast", "pom_batch_step_mixed", "pom_batch_imagine", "pom_batch_deal"):   # one per family unit
        assert getattr(lib, family)(None, None) == 1 and lib.pom_last_error().decode().startswith(family + ": ")
        _fail_another_call(lib)


def test_create_refuses_bad_options_by_name_before_it_needs_a_device(hip_lib):
    """pom_batch_create checks its arguments and options before its first runtime call: each of these is POM_E_ARG with a text of its
    own, with or without a device"""
    from pomcpp_amd.batch import _Options
    lib, size = hip_lib, ctypes.sizeof(_Options)
    out = ctypes.c_void_p()

    def opts(**kw):
        o = _Options(struct_size=size, mode=1)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    assert lib.pom_batch_create(ctypes.byref(out), 64, ctypes.byref(opts(device=1 << 20))) == 2   # good options get as far as the device
    table = [
        ("out is NULL", None, 64, opts()),
        ("n = 0", out, 0, opts()),
        ("n = 2^30 + 1", out, (1 << 30) + 1, opts()),
        ("struct_size 0", out, 64, opts(struct_size=0)),
        ("struct_size sizeof + 8", out, 64, opts(struct_size=size + 8)),
        ("mode 2", out, 64, opts(mode=2)),
        ("auto_reset 3", out, 64, opts(auto_reset=3)),
        ("lanes_per_env 2", out, 64, opts(lanes_per_env=2)),
        ("envs_per_wave 8", out, 64, opts(envs_per_wave=8)),
        ("lanes_per_env 4 with envs_per_wave 32", out, 64, opts(lanes_per_env=4, envs_per_wave=32)),
        ("streams -1", out, 64, opts(streams=-1)),
        ("streams 9", out, 64, opts(streams=9)),
        ("issue_mode 5", out, 64, opts(issue_mode=5)),
        ("RESET_AT_END with lanes_per_env 1", out, 64, opts(auto_reset=2, lanes_per_env=1)),
    ]
    texts = set()
    for what, o, n, op in table:
        assert lib.pom_batch_destroy(None) == 1   # another call's text
        rc = lib.pom_batch_create(None if o is None else ctypes.byref(o), n, ctypes.byref(op))
        text = lib.pom_last_error().decode()
        assert rc == 1 and text.startswith("pom_batch_create: "), (what, rc, text)
        assert not out.value, what
        texts.add(text)
    assert len(texts) >= 10, texts   # (the three bad arguments share a text, the two struct sizes differ in the number only)


def test_product_never_touches_the_oracle():
    """No file of the product (package sources, public headers) includes, links, loads or imports the checker."""
    needles = ("pom_oracle", "libpom_oracle", "oracle_lib", "from tests", "import tests", "oracle/", "_ref")
    for d, _, files in os.walk(os.path.join(ROOT, "pomcpp_amd")):
        for fn in files:
            if fn.endswith((".py", ".h", ".hip", ".cpp", ".hpp")):
                code = open(os.path.join(d, fn)).read()
                code = re.sub(r"/\*.*?\*/", "", code, flags=re.S)      # comments may mention it
                code = re.sub(r'""".*?"""', "", code, flags=re.S)
                code = re.sub(r"#.*", "", code) if fn.endswith(".py") else code
                for n in needles:
                    assert n not in code, (fn, n)
    for fn in os.listdir(os.path.join(ROOT, "include")):
        assert "pom_oracle" not in open(os.path.join(ROOT, "include", fn)).read(), fn
    syms = subprocess.run(["nm", "-D", "--undefined-only", os.path.join(ROOT, "pomcpp_amd", "libpom_batch.so")],
                          capture_output=True, text=True).stdout
    assert "pom_oracle" not in syms and "ref_step" not in syms
