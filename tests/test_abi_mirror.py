"""pomcpp_amd/_abi.py is include/pom_batch.h written a second time by hand: eight ctypes Structures and a table of prototypes.  The
library's struct_size refusal catches a wrong total size, on a GPU; nothing else caught a swapped field or an int64_t passed as 32
bits.  Here the two are compared without the library: sizes and offsets through a C program gcc compiles against the header, names
and prototypes through a parse of the comment-stripped header — and the comparer itself on doctored copies of the mirror."""
import ctypes as C
import os
import re
import subprocess

from pomcpp_amd import _abi
from tests import host_build
from tests.test_cabi import ROOT, _declared_symbols


def _header():
    text = open(os.path.join(ROOT, "include", "pom_batch.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def _header_structs():
    """{name: member names in order} of every `typedef struct NAME { ... } NAME;`"""
    found = re.findall(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", _header(), flags=re.S)
    assert all(tag == name for tag, _, name in found)
    return {name: [re.search(r"(\w+)\s*(?:\[[^\]]*\])?\s*$", m.strip()).group(1) for m in body.split(";") if m.strip()]
            for name, body, _ in found}


def _header_prototypes():
    """{symbol: (return type, parameter declarations)}; `void` is no parameter"""
    found = re.findall(r"^[ \t]*((?:const\s+)?\w+\s*\**)\s*\b(pom_[a-z_]+)\s*\(([^)]*)\)\s*;", _header(), flags=re.M)
    return {name: ("".join(ret.split()), [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in found}


def layout_differences(structures, tmp_path):
    """(a) sizeof of each struct, offsetof and sizeof of each field, as gcc sees the header against what ctypes lays out"""
    lines = []
    for name, cls in structures.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, *_ in cls._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pom_batch.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    try:
        exe = host_build.program(str(src))
    except subprocess.CalledProcessError as e:   # a field the header lacks
        return ["the header does not compile against the mirror's field names: " + e.stderr.strip().splitlines()[0]]
    c_side = dict(line.split(" ", 1) for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines())
    mirror = {}
    for name, cls in structures.items():
        mirror[name] = str(C.sizeof(cls))
        mirror.update({f"{name}.{f}": f"{getattr(cls, f).offset} {getattr(cls, f).size}" for f, *_ in cls._fields_})
    return [f"{k}: the header has {c_side[k]}, the mirror {mirror[k]} (offset size)" for k in mirror if mirror[k] != c_side[k]]


def name_differences(structures):
    """(b) the fields in order are the header's members, and every struct with a struct_size member has a Structure"""
    header = _header_structs()
    specs = {name for name, members in header.items() if "struct_size" in members}
    out = [f"{name}: the header has it, the mirror does not" for name in sorted(specs - set(structures))]
    out += [f"{name}: the mirror has it, the header no such struct with a struct_size" for name in sorted(set(structures) - specs)]
    for name in sorted(specs & set(structures)):
        fields = [f for f, *_ in structures[name]._fields_]
        if fields != header[name]:
            out.append(f"{name}: the header's members are {header[name]}, the mirror's fields {fields}")
    return out


def _is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def _argument_fits(decl, t):
    """(d) does the ctypes type pass what the header's parameter takes"""
    if "*" in decl or "[" in decl:   # `T name[N]` is a pointer parameter
        return _is_pointer(t)
    base = decl.replace("const ", "").split()[0]
    if base in ("int32_t", "int"):
        return isinstance(t, type) and issubclass(t, C._SimpleCData) and C.sizeof(t) == 4 and t(-1).value == -1
    exact = {"int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    return base in exact and t is exact[base]


def prototype_differences(prototypes):
    """(c) the table names exactly the header's symbols with the header's number of arguments, (d) each of a fitting type"""
    header, table = _header_prototypes(), {name: (argtypes, restype) for name, argtypes, restype in prototypes}
    assert sorted(header) == _declared_symbols()   # (the parse finds what tests/test_cabi.py's finds)
    out = [f"{s}: declared in the header, missing from the table" for s in sorted(set(header) - set(table))]
    out += [f"{s}: in the table, not declared in the header" for s in sorted(set(table) - set(header))]
    if len(table) != len(prototypes):
        out.append("a symbol is in the table twice")
    for s in sorted(set(header) & set(table)):
        (ret, params), (argtypes, restype) = header[s], table[s]
        if argtypes is None:
            if params:
                out.append(f"{s}: no argument types for {len(params)} parameters")
        elif len(argtypes) != len(params) or not params:
            out.append(f"{s}: the header has {len(params)} parameters, the table {len(argtypes)} argument types")
        else:
            out += [f"{s}: argument {i} is `{p}`, the table passes {t.__name__}" for i, (p, t) in enumerate(zip(params, argtypes))
                    if not _argument_fits(p, t)]
        want = {"constchar*": (C.c_char_p,), "int64_t": (C.c_int64,)}.get(ret, (None, C.c_int))
        if restype not in want:
            out.append(f"{s}: returns `{ret}`, the table says {restype}")
    return out


def test_structures_have_the_headers_layout(tmp_path):
    assert all(f[0] == "struct_size" for cls in _abi.STRUCTURES.values() for f in cls._fields_[:1])
    assert layout_differences(_abi.STRUCTURES, tmp_path) == []


def test_structures_have_the_headers_members_and_none_is_missing():
    assert name_differences(_abi.STRUCTURES) == []


def test_prototypes_are_the_headers():
    assert prototype_differences(_abi.PROTOTYPES) == []


def _swapped(cls, a, b):
    """`cls` with the fields `a` and `b` in each other's place"""
    fields = [(b if f == a else a if f == b else f, *rest) for f, *rest in cls._fields_]
    return type(cls.__name__, (C.Structure,), {"_fields_": [(f, *rest) for f, *rest in fields]})


def _retyped(name, change):
    return tuple((n, change(list(a)) if n == name else a, r) for n, a, r in _abi.PROTOTYPES)


def test_the_comparer_reports_doctored_mirrors(tmp_path):
    """each of these was the kind of slip nothing caught: the comparer must name it"""
    # src_dev and moves_dev of _ExpandSpec swapped: the same types, so only the names move
    doctored = {**_abi.STRUCTURES, "PomExpandSpec": _swapped(_abi._ExpandSpec, "src_dev", "moves_dev")}
    assert C.sizeof(doctored["PomExpandSpec"]) == C.sizeof(_abi._ExpandSpec)
    got = name_differences(doctored)
    assert len(got) == 1 and got[0].startswith("PomExpandSpec: "), got
    got = layout_differences(doctored, tmp_path)
    assert sorted(d.split(":")[0] for d in got) == ["PomExpandSpec.moves_dev", "PomExpandSpec.src_dev"], got
    # one int64_t argument of pom_batch_upload passed as 32 bits
    def narrowed(a):
        assert a[2] is C.c_int64
        return a[:2] + [C.c_int32] + a[3:]
    got = prototype_differences(_retyped("pom_batch_upload", narrowed))
    assert len(got) == 1 and got[0].startswith("pom_batch_upload: argument 2 "), got
    # one argument dropped from pom_batch_status
    got = prototype_differences(_retyped("pom_batch_status", lambda a: a[:-1]))
    assert len(got) == 1 and got[0].startswith("pom_batch_status: the header has 9 parameters, the table 8"), got
    # and the slips of the other kinds: a ninth spec forgotten, a field the header lacks, a symbol left out, a wrong return type
    got = name_differences({k: v for k, v in _abi.STRUCTURES.items() if k != "PomMoveSafetySpec"})
    assert got == ["PomMoveSafetySpec: the header has it, the mirror does not"], got
    renamed = type("_ViewSpec", (C.Structure,), {"_fields_": [("radius" if f == "view_radius" else f, t) for f, t in _abi._ViewSpec._fields_]})
    got = layout_differences({"PomViewSpec": renamed}, tmp_path)
    assert len(got) == 1 and "does not compile" in got[0], got
    got = prototype_differences(tuple(p for p in _abi.PROTOTYPES if p[0] != "pom_batch_expand"))
    assert got == ["pom_batch_expand: declared in the header, missing from the table"], got
    got = prototype_differences(tuple((n, a, None if n == "pom_batch_size" else r) for n, a, r in _abi.PROTOTYPES))
    assert len(got) == 1 and got[0].startswith("pom_batch_size: returns `int64_t`"), got


def test_batch_still_exports_the_bindings_names():
    from pomcpp_amd import batch
    names = [n for n in vars(_abi) if n.startswith(("MODE_", "RESET_", "DIST_", "CNT_", "ISSUE_", "COPY_", "UB_", "RO_", "ROLLOUT_"))]
    names += [n for n in vars(_abi) if n.endswith("Spec") and n.startswith("_")] + ["_Options", "PomError", "_check", "load_library", "library_path"]
    assert len(names) >= 45 and all(getattr(batch, n) is getattr(_abi, n) for n in names)
