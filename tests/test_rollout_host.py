"""pom_batch_rollout (include/pom_batch.h PomRolloutSpec) without a GPU: the checker (tests/rollout_oracle.py) equals the compiled
reference's playouts (tests/golden/rollout.npz, tests/golden/gen_rollout.py) on every entry, its Python move stream is pom_rng.h's,
the hand-made entries give the words written out by hand below, the header's spec compiles as C and C++ at the size it states, and
the wrapper's structure and decoder agree with it."""
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import rollout_cases as RC
from tests import rollout_oracle as RO
from tests.host_build import ROOT, header_constant, syntax_check

GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout.npz")

# What the hand-made entries of tests/rollout_cases.py must give in every sample, reasoned from the reference's rules.
# finished_game: the IDLE tick before S_0 kills agent 1 (bomb (5, 5), life 1, strength 1, agent on (5, 6)); agents 2 and 3 were dead:
#   aliveAgents == 1, agent 0 wins (environment.cpp:152-163).  The rollout plays nothing: alive 0b0001 | done | winner 0 + 1, length 0.
# three_ticks_left: timeStep 37, max_steps 40.  Nobody can die in three ticks (a bomb planted in tick 1 has 10 ticks to live):
#   alive 0b1111 | done | timed out, no winner, length 3.
HAND = {
    "finished_game": 0x1 | 0x10 | (0 + 1) << 8 | 0 << 16,
    "three_ticks_left": 0xF | 0x10 | 0x40 | 3 << 16,
}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _states(raw):
    return np.ascontiguousarray(raw).view(STATE_DTYPE).reshape(-1)


def test_fixture_holds_the_cases_as_they_are_built(oracle, golden):
    gs = RC.groups()
    assert [g.name for g in gs] == list(golden["names"]), "the cases changed: regenerate tests/golden/rollout.npz"
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert int(golden["seed"]) == RC.SEED and int(golden["samples"]) == RC.SAMPLES
    for i in range(len(RC.KINDS)):
        assert RC.kind_states(oracle, i).tobytes() == golden["states"][i].tobytes()
        assert np.array_equal(RC.kind_moves(i), golden["moves"][i]) and int(golden["dist"][i]) == RC.KINDS[i][2]
    for j, g in enumerate(gs):
        assert (int(golden["kind"][j]), int(golden["horizon"][j]), bool(golden["has_moves"][j])) == (g.kind, g.horizon, g.with_moves)
    hands = RC.hand_made()
    assert [h.name for h in hands] == list(golden["hand_names"]) and set(HAND) == {h.name for h in hands}
    for j, h in enumerate(hands):
        assert h.pre.tobytes() == golden["hand_pre"][j].tobytes()
        assert (h.pre_ticks, h.max_steps, h.horizon) == tuple(int(golden[k][j]) for k in ("hand_pre_ticks", "hand_max_steps", "hand_horizon"))


def test_checker_equals_the_reference_on_every_entry(oracle, golden):
    """the loop over Oracle.step against the same loop over the compiled bboard::Step; and the fixture is not one-sided"""
    res = golden["result"]
    for j, name in enumerate(golden["names"]):
        k = int(golden["kind"][j])
        got = RO.rollout(oracle, _states(golden["states"][k]), int(golden["horizon"][j]), int(golden["samples"]), int(golden["seed"]),
                         int(golden["dist"][k]), golden["moves"][k] if golden["has_moves"][j] else None)
        assert np.array_equal(got, res[j]), name
    length, horizon = res >> RO.RO_LENGTH_SHIFT, golden["horizon"][:, None, None]
    assert 4 * int(((res & RO.RO_DONE != 0) & (length < horizon)).sum()) >= res.size and 4 * int((length == horizon).sum()) >= res.size
    assert int((res >> RO.RO_WINNER_SHIFT & 7 != 0).sum()) >= 10 and (res & RO.RO_DRAW).any() and not (res & RO.RO_UB).any()
    assert not (res & ~np.uint32(0xFFFF07FF)).any()   # the bits the header leaves 0


def test_hand_made_entries(oracle, golden):
    for j, name in enumerate(golden["hand_names"]):
        pre, start = _states(golden["hand_pre"][j]), _states(golden["hand_start"][j])
        max_steps, word = int(golden["hand_max_steps"][j]), 0
        if golden["hand_pre_ticks"][j]:   # S_0 is the pre state after one all-IDLE Environment::Step
            s = pre.copy()
            status = dict(done=0, winner=-1, draw=0)
            oracle.env_step(s, np.zeros(4, dtype=np.int32), status)
            s["agents"]["pad"] = 0
            assert s.tobytes() == start.tobytes() and status["done"] == 1
            word = RO.RO_DONE | (status["winner"] + 1) << RO.RO_WINNER_SHIFT | (RO.RO_DRAW if status["draw"] else 0)
        else:
            assert pre.tobytes() == start.tobytes()
        assert int(golden["hand_start_word"][j]) == word, name
        got = RO.rollout(oracle, start, int(golden["hand_horizon"][j]), int(golden["samples"]), int(golden["seed"]), RO.DIST_RANDOM,
                         max_steps=max_steps, start=golden["hand_start_word"][j:j + 1])
        assert got[:, 0].tolist() == golden["hand_result"][j].tolist() == [HAND[str(name)]] * int(golden["samples"]), name


@pytest.mark.parametrize("dist", [RO.DIST_HARMLESS, RO.DIST_RANDOM, RO.DIST_STRESS])
def test_python_move_stream_is_the_oracles(oracle, dist):
    """five ticks of Oracle.run_random (pom_rng.h compiled) against Oracle.step fed with the Python restatement"""
    import pomcpp_amd as pa
    n, ticks, seed, first_env, tick0 = 12, 5, 0xDEADBEEF12345678, 1000, 7
    start = pa.make_boards(n, seed=4)
    a, b = start.copy(), start.copy()
    oracle.run_random(a, start, ticks, seed, first_env, tick0, dist, 0)
    seen = set()
    for t in range(ticks):
        for e in range(n):
            mv = RO.rng_moves(seed, first_env + e, tick0 + t, dist)
            seen.update(mv)
            oracle.step(b[e:e + 1], mv)
            b["timeStep"][e] += 1
    assert a.tobytes() == b.tobytes()
    assert seen == set(range(5 if dist == RO.DIST_HARMLESS else 6))
    assert RO.splitmix64(0) == 0xE220A8397B1DCDAF   # SplitMix64's published first output for seed 0


SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomRolloutSpec) == POM_ROLLOUT_SPEC_SIZE && POM_ROLLOUT_SPEC_SIZE == 48 ? 1 : -1];
typedef char limits[POM_ROLLOUT_MAX_TICKS == 1024 && POM_ROLLOUT_MAX_SAMPLES == 256 ? 1 : -1];
typedef char offsets[offsetof(PomRolloutSpec, seed) == 16 && offsetof(PomRolloutSpec, moves_dev) == 24 &&
                     offsetof(PomRolloutSpec, result_dev) == 32 && offsetof(PomRolloutSpec, reserved_) == 40 ? 1 : -1];
typedef char word[(POM_RO_ALIVE | POM_RO_DONE | POM_RO_DRAW | POM_RO_TIMEOUT | POM_RO_UB | POM_RO_WINNER_MASK) == 0x7FF &&
                  POM_RO_WINNER_MASK == 7 << POM_RO_WINNER_SHIFT && POM_RO_LENGTH_SHIFT == 16 ? 1 : -1];
int use(PomBatch* h, uint32_t* out)
{
    PomRolloutSpec s = {sizeof(PomRolloutSpec), 32, 16, POM_DIST_RANDOM, 7u, 0, 0, 0};
    s.result_dev = out;
    return pom_batch_rollout(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert header_constant("POM_ROLLOUT_SPEC_SIZE") == 48


def test_wrapper_structure_is_the_headers():
    import ctypes as C
    from pomcpp_amd.batch import _RolloutSpec
    assert C.sizeof(_RolloutSpec) == 48
    assert [getattr(_RolloutSpec, f).offset for f, _ in _RolloutSpec._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert [f for f, _ in _RolloutSpec._fields_] == ["struct_size", "horizon", "samples", "dist", "seed", "moves_dev", "result_dev", "reserved_"]


def test_decode_rollout_inverts_a_packed_word():
    import torch
    from pomcpp_amd import batch as B
    from pomcpp_amd import decode_rollout
    assert (B.RO_DONE, B.RO_DRAW, B.RO_TIMEOUT, B.RO_UB, B.RO_WINNER_SHIFT, B.RO_LENGTH_SHIFT) == \
        (RO.RO_DONE, RO.RO_DRAW, RO.RO_TIMEOUT, RO.RO_UB, RO.RO_WINNER_SHIFT, RO.RO_LENGTH_SHIFT)
    rng = np.random.default_rng(5)
    shape = (3, 7)
    f = {"alive": rng.integers(0, 2, shape + (4,)).astype(bool), "done": rng.integers(0, 2, shape).astype(bool),
         "draw": rng.integers(0, 2, shape).astype(bool), "timeout": rng.integers(0, 2, shape).astype(bool),
         "ub": rng.integers(0, 2, shape).astype(bool), "winner": rng.integers(-1, 4, shape).astype(np.int32),
         "length": rng.integers(0, 1025, shape).astype(np.int32)}
    f["length"][0, 0], f["winner"][0, 0] = 0xFFFF, 3   # the top bit of the word set: int32 input is negative there
    words = ((f["alive"] << np.arange(4)).sum(-1) | f["done"] * 0x10 | f["draw"] * 0x20 | f["timeout"] * 0x40 | f["ub"] * 0x80 |
             (f["winner"] + 1) << 8 | f["length"].astype(np.int64) << 16).astype(np.uint32)
    for given in (words, words.view(np.int32), torch.from_numpy(words.view(np.int32).copy())):
        got = decode_rollout(given)
        assert set(got) == set(f)
        for k, v in f.items():
            g = got[k].numpy() if hasattr(got[k], "numpy") else got[k]
            assert g.dtype == v.dtype and np.array_equal(g, v), k
    assert decode_rollout(np.uint32(HAND["three_ticks_left"]).reshape(1))["length"].tolist() == [3]
