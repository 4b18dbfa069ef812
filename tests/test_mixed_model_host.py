"""The host model of a handle under pom_batch_step_mixed (tests/mixed_model.py) and the schedules of tests/test_step_mixed.py
(tests/mixed_cases.py), without a GPU: the model reduces to the existing ones where the header says the call does (mask 0: RangeModel;
all four agents, whole batch: the checker's SimpleAgent games); it reproduces the golden fixture, every tick of which the compiled
reference played; every schedule contains what can go wrong — asserted from the model alone, so that a change of seed that loses a
condition fails here and not silently on the GPU —; and six deliberately wrong variants of the model, each a mistake the kernel could
make, differ from the model in something MixedModel.same_as compares, in every case in which the mistake can show."""
import os

import numpy as np
import pytest

from tests import mixed_cases as MC
from tests import range_cases as RC
from tests.mixed_model import MixedModel
from tests.range_model import RESET_OFF, RESET_AT_START

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mixed_step.npz")
_played = {}


def _play(oracle, case):
    """the model after the case's schedule, computed once and shared (never changed)"""
    if case["name"] not in _played:
        _played[case["name"]] = MC.play(oracle, case)
    return _played[case["name"]]


# ---- the model is the existing models where the call is the existing calls ------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in MC.CASES if c["mask"] == 0], ids=lambda c: c["name"])
def test_mask_0_is_the_range_model(oracle, case):
    mixed, plain = MC.model_of(oracle, case), RC.model_of(oracle, case)
    plain.states, plain.done, plain.winner, plain.draw = mixed.states.copy(), mixed.done.copy(), mixed.winner.copy(), mixed.draw.copy()
    plain.timeout, plain.ubflags, plain.episodes, plain.finished = mixed.timeout.copy(), mixed.ubflags.copy(), mixed.episodes.copy(), mixed.finished.copy()
    plain.terminal, plain.last, plain.counters = mixed.terminal.copy(), {k: v.copy() for k, v in mixed.last.items()}, mixed.counters.copy()
    for i, moves, tick in MC.schedule(case):
        mixed.tick_mixed(*case["ranges"][i], moves, 0, MC.SEED, tick)
        plain.tick(*case["ranges"][i], moves)
    mine, theirs = mixed.readable(), plain.readable()
    assert all(np.asarray(mine[k]).tobytes() == np.asarray(theirs[k]).tobytes() for k in theirs)


@pytest.mark.parametrize("fresh", [False, True], ids=["snapshot", "fresh"])
def test_all_four_agents_whole_batch_is_the_checkers_simple_game(oracle, fresh):
    n, cap, ticks, tick0 = 40, 12, 30, 9
    case = dict(boards="generated" if fresh else "new", n=n)
    start = RC.boards_of(oracle, case)
    m = MixedModel(oracle, start, max_steps=cap, auto_reset=RESET_AT_START, fresh_boards=fresh, board_seed=RC.BSEED, env_offset=RC.ENV_OFFSET)
    m.handle_tick = tick0
    m.simple_ticks(MC.SEED, ticks)
    want, mems, eps = start.copy(), np.zeros((n, 4, 16), dtype=np.int32), np.zeros(n, dtype=np.int32)
    if fresh:
        oracle.run_simple_fresh(want, eps, mems, ticks, MC.SEED, RC.BSEED, RC.ENV_OFFSET, tick0, cap)
    else:
        oracle.run_simple(want, start, mems, ticks, MC.SEED, RC.ENV_OFFSET, tick0, cap)
    want["agents"]["pad"] = 0
    assert m.counters[2] >= n and m.states.tobytes() == want.tobytes() and np.array_equal(m.mems, mems)
    assert not fresh or np.array_equal(m.episodes, eps)


def test_the_model_reproduces_the_golden_fixture(oracle):
    """every tick of the fixture was played by the compiled reference's Step and every act by its SimpleAgent
    (tests/golden/gen_mixed_step.py)"""
    g = np.load(GOLDEN)
    from pomcpp_amd.state import STATE_DTYPE
    start = g["start"].view(STATE_DTYPE).reshape(-1)
    n, ticks = start.size, g["moves"].shape[0]
    assert n >= 32 and ticks >= 24 and int(g["restarts"]) > 0 and int(g["dead_in_mask"]) > 0
    m = MixedModel(oracle, start, max_steps=int(g["max_steps"]), auto_reset=RESET_AT_START, env_offset=int(g["env_offset"]))
    for t in range(ticks):
        m.tick_mixed(0, n, g["moves"][t], int(g["mask"]), int(g["seed"]), int(g["tick0"]) + t)
        assert m.states.tobytes() == g["states"][t].tobytes(), t
        assert np.array_equal(m.mems, g["mems"][t]), t
    assert m.counters[2] == int(g["restarts"])


# ---- the schedules contain what can go wrong ----------------------------------------------------------------------------------------
def _of_range(case, m, i):
    first, count = case["ranges"][i]
    return [c for c in m.calls[m.before["calls"]:] if (c["first"], c["count"]) == (first, count)]


@pytest.mark.parametrize("case", MC.CASES, ids=MC.CASE_IDS)
def test_schedule_contains_what_can_go_wrong(oracle, case):
    m = _play(oracle, case)
    k, mask = len(case["ranges"]), case["mask"]
    per_range = [_of_range(case, m, i) for i in range(k)]
    assert all(len(calls) >= 4 for calls in per_range) and len({len(calls) for calls in per_range}) > 1, "the ranges stand at different ticks"
    mixed_calls = m.calls[m.before["calls"]:]
    assert any((a["first"], a["count"]) == (b["first"], b["count"]) for a, b in zip(mixed_calls, mixed_calls[1:])), "no range is called twice in a row"
    # every agent has memory when the first mixed call comes, the agents outside the mask included
    outside = [a for a in range(4) if not mask >> a & 1]
    assert all((m.before["memory"][:, a] != 0).any(axis=1).mean() > 0.5 for a in range(4)), "agents without memory before the first mixed call"
    assert not outside or (m.before["memory"][:, outside] != 0).any()
    if case["reset"] == RESET_OFF:
        assert any(c["skipped"] for c in mixed_calls) and m.counters[2] == 0, "no finished env is skipped"
    else:
        for i, calls in enumerate(per_range):
            assert any(c["restarted"] for c in calls), f"range {i} never restarts an env"
    if case["boards"] in ("burned", "crowded") and mask:
        assert sum(c["dead_in_mask"] for c in mixed_calls) > 0, "no env with a dead agent of the mask is played"
    if case["boards"] == "stress":
        assert sum(c["ub"] for c in mixed_calls) > 0, "no UB tick"


def test_the_cases_cover_every_mode_and_mask():
    assert {(c["reset"], c["fresh"], c["mask"]) for c in MC.CASES} >= {(r, f, k) for r, f in RC.MODES for k in MC.MASKS}
    assert any(c["n"] == RC.SMALL_N for c in MC.CASES) and MC.MASKS == (0b1110, 0b0101, 0xF, 0)


@pytest.mark.parametrize("case", MC.STREAM_CASES, ids=lambda c: c["name"])
def test_stream_schedule_restarts_in_every_range(oracle, case):
    m = MC.model_of(oracle, case)
    before = len(m.calls)
    for a, b in MC.stream_schedule(case):
        for i, moves, tick in a + b:
            m.tick_mixed(*case["ranges"][i], moves, case["mask"], MC.SEED, tick)
    for first, count in case["ranges"]:
        assert any(c["restarted"] for c in m.calls[before:] if (c["first"], c["count"]) == (first, count)), (first, count)


# ---- the schedules tell a wrong kernel from a right one ---------------------------------------------------------------------------------
class MemoryNotWipedOnRestart(MixedModel):
    def _wipe(self, e):
        pass


class AgentOutsideTheMaskAsked(MixedModel):
    def _kept(self, mask):
        return 15


class DrawKeyedByIndexInTheRange(MixedModel):
    def _draw_env(self, e, first):
        return self.env_offset + e - first


class DrawKeyedByTheHandlesTick(MixedModel):
    def _draw_tick(self, tick):
        return self.handle_tick


class MaskAgentsMoveFromTheCaller(MixedModel):
    def _select(self, e, a, in_mask, dead, policy_move, callers_move):
        return callers_move


class DeadMaskAgentNotIdle(MixedModel):
    def _select(self, e, a, in_mask, dead, policy_move, callers_move):
        return callers_move if in_mask and dead else super()._select(e, a, in_mask, dead, policy_move, callers_move)


WRONG = [  # (variant, the cases it can show in, what must differ at least)
    (MemoryNotWipedOnRestart, lambda c: c["reset"] != RESET_OFF, "memory"),
    (AgentOutsideTheMaskAsked, lambda c: c["mask"] not in (0, 15), "memory"),
    (DrawKeyedByIndexInTheRange, lambda c: c["mask"] != 0, "memory"),
    (DrawKeyedByTheHandlesTick, lambda c: c["mask"] != 0, "memory"),
    (MaskAgentsMoveFromTheCaller, lambda c: c["mask"] != 0, "state"),
    (DeadMaskAgentNotIdle, lambda c: c["boards"] == "crowded", "state"),   # (elsewhere a dead agent's entry rarely decides anything)
]


@pytest.mark.parametrize("variant,applies,field", WRONG, ids=[w[0].__name__ for w in WRONG])
def test_wrong_variants_are_told_apart(oracle, variant, applies, field):
    """in EVERY case in which the mistake can show it does show, in something same_as compares"""
    cases = [c for c in MC.CASES if applies(c)]
    assert len(cases) >= (2 if variant is DeadMaskAgentNotIdle else 10)
    shown_in_field = 0
    for case in cases:
        right, wrong = _play(oracle, case), MC.play(oracle, case, variant)
        assert right.differences(wrong), f"{variant.__name__} passes for the model in {case['name']}"
        shown_in_field += field in right.differences(wrong)
    assert shown_in_field >= len(cases) - 2, (variant.__name__, field, shown_in_field, len(cases))   # (a low max_steps wipes most traces)
