"""pom_batch_expand (include/pom_batch.h PomExpandSpec) without a GPU: the header's spec compiles as C and C++ at the size and offsets
it states, the older specs are the size they were, the wrapper's structure agrees with the header, the library exports the call, the
spec's checks answer before the handle is touched, and the checker (tests/expand_oracle.py) replays the compiled reference's steps
(tests/golden/step_cases.npz): every `__before` with its `__moves` gives `__after`."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import expand_oracle as XO
from tests.host_build import ROOT, syntax_check

GOLDEN = os.path.join(ROOT, "tests", "golden", "step_cases.npz")

OFFSETS = dict(struct_size=0, flags=4, first=8, count=16, src_dev=24, moves_dev=32, result_dev=40, planes_dev=48, dtype=56, per_agent=60,
               agent_attrs_dev=64, env_attrs_dev=72, reserved_=80)

SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomExpandSpec) == POM_EXPAND_SPEC_SIZE && POM_EXPAND_SPEC_SIZE == 88 ? 1 : -1];
typedef char offsets[%s ? 1 : -1];
typedef char no_job[POM_RO_NONE == 0 ? 1 : -1];
typedef char the_older_specs_are_as_they_were[sizeof(PomRolloutSpec) == 48 && POM_ROLLOUT_SPEC_SIZE == 48 &&
                                              sizeof(PomRolloutPolicySpec) == 56 && POM_ROLLOUT_POLICY_SPEC_SIZE == 56 &&
                                              sizeof(PomRolloutJobsSpec) == 72 && POM_ROLLOUT_JOBS_SPEC_SIZE == 72 &&
                                              sizeof(PomForecastSpec) == 48 && POM_FORECAST_SPEC_SIZE == 48 &&
                                              sizeof(PomViewSpec) == 40 && POM_VIEW_SPEC_SIZE == 40 ? 1 : -1];
int use(PomBatch* h, const int64_t* src, const int32_t* moves, uint32_t* out, void* codes)
{
    PomExpandSpec s = {sizeof(PomExpandSpec), 0, 19, 18, 0, 0, 0, 0, POM_OBS_CODES, 0, 0, 0, 0};
    s.src_dev = src;
    s.moves_dev = moves;
    s.result_dev = out;
    s.planes_dev = codes;
    return pom_batch_expand(h, &s);
}
""" % " && ".join(f"offsetof(PomExpandSpec, {f}) == {o}" for f, o in OFFSETS.items())


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)


def test_cpp_wrapper_has_the_call(tmp_path):
    syntax_check('#include "pom_bboard.hpp"\nvoid use(bboard::BatchEnvironment& b, const PomExpandSpec& s) { b.Expand(s); }\n',
                            tmp_path, "g++", "-std=c++17")


def test_wrapper_structure_is_the_headers():
    from pomcpp_amd import batch as B
    S = B._ExpandSpec
    assert C.sizeof(S) == 88 and B.RO_NONE == 0
    assert [f for f, _ in S._fields_] == list(OFFSETS)
    assert [getattr(S, f).offset for f, _ in S._fields_] == list(OFFSETS.values())
    assert C.sizeof(B._RolloutSpec) == 48 and C.sizeof(B._RolloutPolicySpec) == 56 and C.sizeof(B._RolloutJobsSpec) == 72
    assert callable(B.BatchEnvironment.expand)


def test_spec_checks_come_before_the_handle(hip_lib):
    """POM_E_ARG with a text naming the call, and no device anywhere: none of these gets as far as the handle (a null handle is itself
    refused, after the spec's own fields)"""
    from pomcpp_amd.batch import _ExpandSpec as Spec
    lib = hip_lib
    assert hasattr(lib, "pom_batch_expand")                # exported
    lib.pom_last_error.restype = C.c_char_p
    size, p = C.sizeof(Spec), 4096                          # (a pointer nobody follows)

    def spec(**kw):
        f = dict(struct_size=size, flags=0, first=19, count=18, src_dev=p, moves_dev=p, result_dev=p, planes_dev=None, dtype=0, per_agent=0,
                 agent_attrs_dev=None, env_attrs_dev=None, reserved_=0)
        f.update(kw)
        return Spec(*[f[k] for k in OFFSETS])

    bad = {
        "the spec is NULL": None,
        "struct_size": spec(struct_size=size - 8),
        "struct_size ": spec(struct_size=72),
        "flags": spec(flags=1),
        "flags ": spec(flags=-1),
        "reserved_": spec(reserved_=1),
        "count": spec(count=-1),
        "src_dev is NULL": spec(src_dev=None),
        "moves_dev is NULL": spec(moves_dev=None),
        "src_dev must be 8-byte aligned": spec(src_dev=p + 4),
        "moves_dev must be 4-byte aligned": spec(moves_dev=p + 2),
        "result_dev must be 4-byte aligned": spec(result_dev=p + 2),
        "dtype": spec(planes_dev=p, dtype=4),
        "dtype ": spec(planes_dev=p, dtype=-1),
        "the handle is NULL": spec(),
        "the handle is NULL ": spec(result_dev=None),      # the words are optional
        "the handle is NULL  ": spec(count=0, src_dev=None, moves_dev=None, result_dev=None),
    }
    for what, s in bad.items():
        rc = lib.pom_batch_expand(None, None if s is None else C.byref(s))
        text = lib.pom_last_error().decode()
        assert rc == 1 and text.startswith("pom_batch_expand: ") and what.strip() in text, (what, rc, text)


def test_checker_replays_the_golden_steps(oracle):
    """every recorded Step of the compiled reference, as an expansion: the `__before` states in the lower half, their children in the
    upper half through a permuted list; RAW mode is the bare Step, and the sources stay as they were"""
    g = np.load(GOLDEN)
    names = sorted(k[:-len("__before")] for k in g.files if k.endswith("__before"))
    before = np.concatenate([g[f"{k}__before"] for k in names]).view(STATE_DTYPE).reshape(-1)
    after = np.concatenate([g[f"{k}__after"] for k in names]).view(STATE_DTYPE).reshape(-1)
    moves = np.concatenate([g[f"{k}__moves"] for k in names]).astype(np.int32)
    m = before.size
    assert m == 219 and len(names) == 48
    perm = np.random.default_rng(5).permutation(m)
    states = np.concatenate([before, np.zeros(m, dtype=STATE_DTYPE)])
    out, _, words, ticks, _ = XO.expand(oracle, states, None, perm.astype(np.int64), moves[perm], m, XO.MODE_RAW)
    assert out[m:].tobytes() == after[perm].tobytes() and out[:m].tobytes() == before.tobytes()
    assert ticks == m and ((words >> XO.RO_LENGTH_SHIFT) == 1).all() and not (words & (XO.RO_DONE | XO.RO_DRAW | XO.RO_TIMEOUT | 0x700)).any()
    # the no-job rules: below 0, from n on, and another slot of the range — but a slot's own index is a job
    src = np.array([-1, 2 * m, 1 << 40, m + 4, m + 4, 0], dtype=np.int64)
    out2, _, w2, t2, _ = XO.expand(oracle, out, None, src, moves[:6], m, XO.MODE_ENV)
    assert t2 == 2 and not w2[:4].any() and w2[4] and w2[5] and out2[m:m + 4].tobytes() == out[m:m + 4].tobytes()
    assert int(out2["timeStep"][m + 4]) == int(out["timeStep"][m + 4]) + 1 and int(out2["timeStep"][m + 5]) == int(before["timeStep"][0]) + 1
