"""pom_batch_rollout_jobs (include/pom_batch.h PomRolloutJobsSpec) without a GPU: the checker (tests/rollout_jobs_oracle.py) indexes the
compiled reference's playouts (tests/golden/rollout_policy.npz) by source, an identity list is the policy rollout's checker, the
header's spec compiles as C and C++ at the size and offsets it states, the wrapper's structure agrees with it, the library exports
the call, and the spec's checks answer before the handle is touched."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests import rollout_jobs_oracle as JO
from tests import rollout_oracle as RO
from tests import rollout_policy_oracle as PO
from tests.host_build import ROOT, syntax_check

GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout_policy.npz")


def test_checker_on_the_golden_file(oracle):
    """all 18 groups: job j, given moves[src[j]], is the compiled reference's column src[j]"""
    g = np.load(GOLDEN)
    assert len(g["names"]) == 18
    words = 0
    for j, name in enumerate(g["names"]):
        k, fm = int(g["kind"][j]), int(g["first_mask"][j])
        states = np.ascontiguousarray(g["states"][k]).view(STATE_DTYPE).reshape(-1)
        src = JO.golden_jobs(states.size)
        assert states.size == 24 and len(set(src.tolist())) < src.size
        got = JO.rollout_jobs(oracle, states, None, src, int(g["horizon"][j]), int(g["samples"]), int(g["seed"]), int(g["dist"][k]),
                              int(g["simple_mask"][j]), fm, g["moves"][k][src] if fm else None)
        assert np.array_equal(got, g["result"][j][:, src]), name
        words += got.size
    assert words == 18 * 4 * 37


@pytest.mark.parametrize("kind,ticks,dist", [("ffa", 57, RO.DIST_RANDOM), ("stress", 23, RO.DIST_STRESS)])
def test_identity_list_is_the_policy_rollouts_checker(oracle, kind, ticks, dist):
    """... on the whole array, with a stream key that does not start at 0, a step bound and carried memory; and the entries without a
    job give zeros, which no job gives"""
    n, R, K = 12, 2, 24
    states, moves, mems = FC.played_states(oracle, kind, n, ticks), FC.random_moves(n, 3), None
    if kind == "ffa":   # games in the middle of SimpleAgent play, with the memory their agents have by then
        import pomcpp_amd as pa
        states, mems = pa.make_boards(n, seed=21), PO.fresh_memory(n)
        oracle.run_simple(states, states.copy(), mems, 40, 3, 0, 0, 0)
        assert mems.any()
    whole = PO.rollout(oracle, states, mems, K, R, 5, dist, 0xE, 0x3, moves, 70, 1000)
    assert np.array_equal(JO.rollout_jobs(oracle, states, mems, np.arange(n), K, R, 5, dist, 0xE, 0x3, moves, 70, 1000), whole)
    src = np.array([3, -1, n, 3, 1 << 40, 0], dtype=np.int64)
    got = JO.rollout_jobs(oracle, states, mems, src, K, R, 5, dist, 0xE, 0x3, moves[np.clip(src, 0, n - 1)], 70, 1000)
    ok = (src >= 0) & (src < n)
    assert np.array_equal(got[:, ok], whole[:, src[ok]]) and not got[:, ~ok].any() and whole.all() and JO.RO_NONE == 0


SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomRolloutJobsSpec) == POM_ROLLOUT_JOBS_SPEC_SIZE && POM_ROLLOUT_JOBS_SPEC_SIZE == 72 ? 1 : -1];
typedef char offsets[offsetof(PomRolloutJobsSpec, struct_size) == 0 && offsetof(PomRolloutJobsSpec, horizon) == 4 &&
                     offsetof(PomRolloutJobsSpec, samples) == 8 && offsetof(PomRolloutJobsSpec, dist) == 12 &&
                     offsetof(PomRolloutJobsSpec, seed) == 16 && offsetof(PomRolloutJobsSpec, jobs) == 24 &&
                     offsetof(PomRolloutJobsSpec, src_dev) == 32 && offsetof(PomRolloutJobsSpec, moves_dev) == 40 &&
                     offsetof(PomRolloutJobsSpec, result_dev) == 48 && offsetof(PomRolloutJobsSpec, simple_mask) == 56 &&
                     offsetof(PomRolloutJobsSpec, first_mask) == 60 && offsetof(PomRolloutJobsSpec, flags) == 64 &&
                     offsetof(PomRolloutJobsSpec, reserved_) == 68 ? 1 : -1];
typedef char no_job[POM_RO_NONE == 0 ? 1 : -1];
typedef char the_older_specs_are_as_they_were[sizeof(PomRolloutSpec) == 48 && POM_ROLLOUT_SPEC_SIZE == 48 &&
                                              sizeof(PomRolloutPolicySpec) == 56 && POM_ROLLOUT_POLICY_SPEC_SIZE == 56 ? 1 : -1];
int use(PomBatch* h, const int64_t* src, const int32_t* moves, uint32_t* out)
{
    PomRolloutJobsSpec s = {sizeof(PomRolloutJobsSpec), 32, 16, POM_DIST_RANDOM, 7u, 96, 0, 0, 0, 0xE, 0x1, POM_ROLLOUT_FRESH_AGENTS, 0};
    s.src_dev = src;
    s.moves_dev = moves;
    s.result_dev = out;
    return pom_batch_rollout_jobs(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)


def test_cpp_wrapper_has_the_call(tmp_path):
    syntax_check('#include "pom_bboard.hpp"\nvoid use(bboard::BatchEnvironment& b, const PomRolloutJobsSpec& s) { b.RolloutJobs(s); }\n',
                            tmp_path, "g++", "-std=c++17")


def test_wrapper_structure_is_the_headers():
    from pomcpp_amd import batch as B
    S = B._RolloutJobsSpec
    assert C.sizeof(S) == 72 and B.RO_NONE == 0
    assert [f for f, _ in S._fields_] == ["struct_size", "horizon", "samples", "dist", "seed", "jobs", "src_dev", "moves_dev", "result_dev",
                                          "simple_mask", "first_mask", "flags", "reserved_"]
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 60, 64, 68]
    assert C.sizeof(B._RolloutSpec) == 48 and C.sizeof(B._RolloutPolicySpec) == 56
    assert callable(B.BatchEnvironment.rollout_jobs) and callable(B.BatchEnvironment.move_table)


def test_spec_checks_come_before_the_handle(hip_lib):
    """POM_E_ARG with a text naming the call, and no device anywhere: none of these gets as far as the handle (a null handle is itself
    refused, after the spec's own fields)"""
    from pomcpp_amd.batch import _RolloutJobsSpec as Spec
    lib = hip_lib
    assert hasattr(lib, "pom_batch_rollout_jobs")          # exported
    lib.pom_last_error.restype = C.c_char_p
    size, p = C.sizeof(Spec), 4096                          # (a pointer nobody follows)
    good = Spec(size, 8, 2, 1, 7, 37, p, p, p, 0xE, 0x1, 0, 0)
    bad = {
        "the spec is NULL": None,
        "struct_size": Spec(size - 8, 8, 2, 1, 7, 37, p, p, p, 0xE, 0x1, 0, 0),
        "struct_size ": Spec(56, 8, 2, 1, 7, 37, p, p, p, 0xE, 0x1, 0, 0),
        "simple_mask": Spec(size, 8, 2, 1, 7, 37, p, p, p, 16, 0x1, 0, 0),
        "simple_mask ": Spec(size, 8, 2, 1, 7, 37, p, p, p, -1, 0x1, 0, 0),
        "first_mask": Spec(size, 8, 2, 1, 7, 37, p, p, p, 0xE, 16, 0, 0),
        "first_mask ": Spec(size, 8, 2, 1, 7, 37, p, p, p, 0xE, -1, 0, 0),
        "flags": Spec(size, 8, 2, 1, 7, 37, p, p, p, 0xE, 0x1, 2, 0),
        "flags ": Spec(size, 8, 2, 1, 7, 37, p, p, p, 0xE, 0x1, -1, 0),
        "reserved_": Spec(size, 8, 2, 1, 7, 37, p, p, p, 0xE, 0x1, 0, 1),
        "jobs": Spec(size, 8, 2, 1, 7, -1, p, p, p, 0xE, 0x1, 0, 0),
        "moves_dev is NULL": Spec(size, 8, 2, 1, 7, 37, p, None, p, 0xE, 0x1, 0, 0),
        "src_dev is NULL": Spec(size, 8, 2, 1, 7, 37, None, p, p, 0xE, 0x1, 0, 0),
        "src_dev must be 8-byte aligned": Spec(size, 8, 2, 1, 7, 37, p + 4, p, p, 0xE, 0x1, 0, 0),
        "the handle is NULL": good,
    }
    for what, spec in bad.items():
        rc = lib.pom_batch_rollout_jobs(None, None if spec is None else C.byref(spec))
        text = lib.pom_last_error().decode()
        assert rc == 1 and text.startswith("pom_batch_rollout_jobs: ") and what.strip() in text, (what, rc, text)
