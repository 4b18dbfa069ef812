"""pom_batch_rollout_policy (include/pom_batch.h PomRolloutPolicySpec) without a GPU: the checker (tests/rollout_policy_oracle.py)
equals the compiled reference's playouts (tests/golden/rollout_policy.npz, tests/golden/gen_rollout_policy.py) on every entry, without
SimpleAgents it is the rollout's checker, with four fresh ones it is Oracle.run_simple plus the bookkeeping, the header's spec compiles
as C and C++ at the size and offsets it states, and the wrapper's structure agrees with it."""
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests import rollout_oracle as RO
from tests import rollout_policy_cases as PC
from tests import rollout_policy_oracle as PO
from tests.host_build import ROOT, header_constant, syntax_check

GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout_policy.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _states(raw):
    return np.ascontiguousarray(raw).view(STATE_DTYPE).reshape(-1)


def test_fixture_holds_the_cases_as_they_are_built(oracle, golden):
    gs = PC.groups()
    assert [g.name for g in gs] == list(golden["names"]), "the cases changed: regenerate tests/golden/rollout_policy.npz"
    assert len(gs) == 18 and os.path.getsize(GOLDEN) < 256 * 1024
    assert int(golden["seed"]) == PC.SEED and int(golden["samples"]) == PC.SAMPLES == 4 and PC.PER_KIND == 24
    assert {(g.simple_mask, g.first_mask) for g in gs} == {(0xF, 0), (0xE, 0), (0xE, 1)} and {g.horizon for g in gs} == {1, 8, 48}
    for i in range(len(PC.KINDS)):
        assert PC.kind_states(oracle, i).tobytes() == golden["states"][i].tobytes()
        assert np.array_equal(PC.kind_moves(i), golden["moves"][i]) and int(golden["dist"][i]) == PC.KINDS[i][2]
    for j, g in enumerate(gs):
        assert tuple(int(golden[k][j]) for k in ("kind", "horizon", "simple_mask", "first_mask")) == (g.kind, g.horizon, g.simple_mask, g.first_mask)


def test_checker_equals_the_reference_on_every_entry(oracle, golden):
    """the loop over Oracle.simple_policy and Oracle.step against the same loop over the compiled SimpleAgent::act and bboard::Step; and
    the fixture as a whole is not one-sided"""
    res = golden["result"]
    for j, name in enumerate(golden["names"]):
        k, fm = int(golden["kind"][j]), int(golden["first_mask"][j])
        got = PO.rollout(oracle, _states(golden["states"][k]), None, int(golden["horizon"][j]), int(golden["samples"]), int(golden["seed"]),
                         int(golden["dist"][k]), int(golden["simple_mask"][j]), fm, golden["moves"][k] if fm else None)
        assert np.array_equal(got, res[j]), name
    a0_alive = np.stack([_states(golden["states"][int(k)])["agents"]["dead"][:, 0] == 0 for k in golden["kind"]])
    size, early, full, winners, draws, a0_dies = bal = PC.balance(res, golden["horizon"], a0_alive)
    assert 8 * early >= size and 8 * full >= size and winners >= 10 and draws >= 1 and a0_dies >= 10, bal
    assert not (res & RO.RO_UB).any() and not (res & ~np.uint32(0xFFFF07FF)).any()   # no flag; the bits the header leaves 0


@pytest.mark.parametrize("kind,ticks,dist", [("ffa", 57, RO.DIST_RANDOM), ("stress", 23, RO.DIST_STRESS)])
def test_without_simple_agents_it_is_the_rollouts_checker(oracle, kind, ticks, dist):
    n, R, K = 16, 2, 24
    states, moves = FC.played_states(oracle, kind, n, ticks), FC.random_moves(n, 3)
    junk = np.full((n, 4, 16), 3, dtype=np.int32)   # nobody reads the memory
    assert np.array_equal(PO.rollout(oracle, states, junk, K, R, 5, dist, 0, max_steps=70, env_offset=40),
                          RO.rollout(oracle, states, K, R, 5, dist, None, 70, 40))
    assert np.array_equal(PO.rollout(oracle, states, None, K, R, 5, dist, 0, 0xF, moves, env_offset=40),
                          RO.rollout(oracle, states, K, R, 5, dist, moves, env_offset=40))


@pytest.mark.parametrize("kind,ticks", [("ffa", 57), ("stress", 23)])
def test_four_fresh_simple_agents_are_run_simple_plus_the_bookkeeping(oracle, kind, ticks):
    """pom_oracle_run_simple (the C loop behind the step_simple tests) one tick at a time on every env until its game is over"""
    n, R, K, seed, off, max_steps = 24, 2, 48, 11, 1000, 90
    states = FC.played_states(oracle, kind, n, ticks)
    got = PO.rollout(oracle, states, None, K, R, seed, RO.DIST_RANDOM, 0xF, max_steps=max_steps, env_offset=off)
    want = np.zeros_like(got)
    for r in range(R):
        seed_r = RO.splitmix64(seed + r)
        for e in range(n):
            s, m = states[e:e + 1].copy(), PO.fresh_memory(1)
            word = length = 0
            while length < K and not word & RO.RO_DONE:
                # run_simple's own restart rule is kept out of it: max_steps 0, and a game that is over is not stepped again.  A
                # board with one agent left at S_0 "restarts" as itself with the fresh agents it has anyway
                assert length == 0 or int(s["aliveAgents"][0]) > 1
                oracle.run_simple(s, s.copy(), m, 1, seed_r, off + e, length, 0)
                length += 1
                alive = int(s["aliveAgents"][0])
                if alive == 1:
                    word |= RO.RO_DONE | (max(a for a in range(4) if not s["agents"][0, a]["dead"]) + 1) << RO.RO_WINNER_SHIFT
                if alive == 0:
                    word |= RO.RO_DONE | RO.RO_DRAW
                if int(s["timeStep"][0]) >= max_steps:
                    word |= RO.RO_DONE | RO.RO_TIMEOUT
            want[r, e] = word | RO.alive_bits(s) | length << RO.RO_LENGTH_SHIFT
    ub = (got & RO.RO_UB) != 0   # (run_simple does not return the flags)
    assert np.array_equal(got & ~np.uint32(RO.RO_UB), want)
    assert (want & RO.RO_DONE).any() and (want & RO.RO_DONE == 0).any() and ub.sum() < ub.size


def test_carried_memory_matters(oracle):
    """the checker started from the memory the agents have after 40 ticks differs from the checker started with fresh agents"""
    import pomcpp_amd as pa
    n = 48
    s, m = pa.make_boards(n, seed=21), PO.fresh_memory(n)
    oracle.run_simple(s, s.copy(), m, 40, 3, 0, 0, 0)
    assert m.any()
    carried, fresh = (PO.rollout(oracle, s, mem, 24, 2, 7, RO.DIST_RANDOM, 0xF) for mem in (m, None))
    assert (carried != fresh).any()


SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomRolloutPolicySpec) == POM_ROLLOUT_POLICY_SPEC_SIZE && POM_ROLLOUT_POLICY_SPEC_SIZE == 56 ? 1 : -1];
typedef char offsets[offsetof(PomRolloutPolicySpec, seed) == 16 && offsetof(PomRolloutPolicySpec, moves_dev) == 24 &&
                     offsetof(PomRolloutPolicySpec, result_dev) == 32 && offsetof(PomRolloutPolicySpec, simple_mask) == 40 &&
                     offsetof(PomRolloutPolicySpec, first_mask) == 44 && offsetof(PomRolloutPolicySpec, flags) == 48 &&
                     offsetof(PomRolloutPolicySpec, reserved_) == 52 ? 1 : -1];
typedef char flag[POM_ROLLOUT_FRESH_AGENTS == 1 ? 1 : -1];
typedef char the_old_spec_is_as_it_was[sizeof(PomRolloutSpec) == 48 && POM_ROLLOUT_SPEC_SIZE == 48 ? 1 : -1];
int use(PomBatch* h, uint32_t* out, const int32_t* moves)
{
    PomRolloutPolicySpec s = {sizeof(PomRolloutPolicySpec), 32, 16, POM_DIST_RANDOM, 7u, 0, 0, 0xE, 0x1, POM_ROLLOUT_FRESH_AGENTS, 0};
    s.moves_dev = moves;
    s.result_dev = out;
    return pom_batch_rollout_policy(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert header_constant("POM_ROLLOUT_POLICY_SPEC_SIZE") == 56


def test_wrapper_structure_is_the_headers():
    import ctypes as C
    from pomcpp_amd import batch as B
    S = B._RolloutPolicySpec
    assert C.sizeof(S) == 56 and B.ROLLOUT_FRESH_AGENTS == 1
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 44, 48, 52]
    assert [f for f, _ in S._fields_] == ["struct_size", "horizon", "samples", "dist", "seed", "moves_dev", "result_dev", "simple_mask",
                                          "first_mask", "flags", "reserved_"]
    assert B._agent_mask(0xE, "simple") == 0xE and B._agent_mask([1, 2, 3], "simple") == 0xE and B._agent_mask((), "first") == 0
    for bad in (16, -1, [4], [-1], 1.5):
        with pytest.raises(ValueError):
            B._agent_mask(bad, "simple")
