"""The host model of a handle under range ticks (tests/range_model.py) and the schedules of tests/test_range_modes.py
(tests/range_cases.py), without a GPU: the model is the existing replay (tests/test_visit_path.replay) when every range is ticked once
per round; every schedule contains what it is there for — asserted from the model alone, so that a change of seed that loses a
condition fails here and not silently on the GPU —; and five deliberately wrong variants of the model, each the mistake a range kernel
could make without any older test noticing, differ from the model in something RangeModel.same_as compares on those schedules."""
import numpy as np
import pytest

from pomcpp_amd.batch import DIST_RANDOM
from tests import range_cases as RC
from tests.range_model import RangeModel, RESET_OFF, RESET_AT_START, RESET_AT_END

_played = {}


def _play(oracle, case):
    """the model after the case's schedule, computed once and shared (never changed)"""
    if case["name"] not in _played:
        _played[case["name"]] = RC.play(oracle, case)
    return _played[case["name"]]


# ---- the model is the existing replay ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [3, 800])
@pytest.mark.parametrize("how", ["snapshot", "fresh", "at_end"])
def test_every_range_once_per_round_is_the_replay(oracle, how, cap):
    from tests.test_visit_path import replay, BSEED, ENV_OFFSET, SEED, TICK0
    assert (BSEED, ENV_OFFSET) == (RC.BSEED, RC.ENV_OFFSET)
    n, ticks, fresh, at_end = RC.SMALL_N, 40, how == "fresh", how == "at_end"
    case = dict(boards=("generated" if fresh else "new") if cap == 3 else "burned", n=n)
    start = RC.boards_of(oracle, case)
    tape = np.zeros((ticks, n, 4), dtype=np.int32)
    states, counters, flags = replay(oracle, start, ticks, DIST_RANDOM, cap, fresh=fresh, at_end=at_end, moves_out=tape)
    assert counters[-1][2] > 0, "precondition: the replay restarts somebody"
    m = RangeModel(oracle, start, max_steps=cap, auto_reset=RESET_AT_END if at_end else RESET_AT_START, fresh_boards=fresh,
                   board_seed=BSEED, env_offset=ENV_OFFSET)
    twin = RangeModel(oracle, start, max_steps=cap, auto_reset=RESET_AT_END if at_end else RESET_AT_START, fresh_boards=fresh,
                      board_seed=BSEED, env_offset=ENV_OFFSET)
    for t in range(ticks):
        for first, count in (RC.SMALL_RANGES if t % 2 else RC.SMALL_RANGES[::-1]):
            m.tick(first, count, tape[t])
        assert m.states.tobytes() == states[t].tobytes(), (how, cap, t)
        assert m.counters.tolist() == counters[t].tolist(), (how, cap, t)
    # random_ticks is the same replay, the moves drawn here
    twin.random_ticks(SEED, DIST_RANDOM, TICK0, ticks)
    assert not m.differences(twin)


# ---- the schedules contain what they are there for ------------------------------------------------------------------------------
def _of_range(case, m, i):
    first, count = case["ranges"][i]
    return [c for c in m.calls if (c["first"], c["count"]) == (first, count)]


@pytest.mark.parametrize("case", RC.CASES, ids=RC.CASE_IDS)
def test_schedule_contains_what_it_is_there_for(oracle, case):
    m = _play(oracle, case)
    k = len(case["ranges"])
    per_range = [_of_range(case, m, i) for i in range(k)]
    assert all(len(calls) >= RC.ROUNDS // 2 for calls in per_range), "every range is called in most rounds"
    assert any((a["first"], a["count"]) == (b["first"], b["count"]) for a, b in zip(m.calls, m.calls[1:])), "no range is called twice in a row"
    assert len({len(calls) for calls in per_range}) > 1, "the ranges stand at different ticks"
    ticked = sum(c["ticked"] for c in m.calls)
    assert m.counters[0] == ticked > 0
    if case["reset"] == RESET_OFF:
        assert m.counters[2] == 0 and m.counters[1] > 0 and m.done.any(), "some env finishes and stays finished"
        assert ticked < sum(c["count"] for c in m.calls), "some call skips a finished env"
        return
    for i, calls in enumerate(per_range):
        assert any(c["restarted"] for c in calls), f"range {i} never restarts an env"
    if case["reset"] == RESET_AT_END:
        assert any(c["marked_outside"] for c in m.calls), "no call finds a `finished` mark of an earlier call outside its range"
    if case["cap"] == 3:
        tiles = [np.bincount(np.asarray(c["restarted"]) // 16, minlength=case["n"] // 16 + 1) for c in m.calls if c["restarted"]]
        assert any((t == 16).any() for t in tiles), "no call restarts all 16 envs of a tile"
    if case["cap"] == 800:
        assert sum(c["by_deaths"] for c in m.calls) >= 1, "no game ends by deaths"
        assert m.counters[2] < ticked / 4, "a quarter or more of the env-ticks restart"
    if case["fresh"]:
        ep = m.episodes.astype(np.int64)
        assert ep.sum() == m.counters[2]
        assert len({float(ep[f:f + c].mean()) for f, c in case["ranges"]}) == k, "the ranges' episode numbers do not differ"
    if case["boards"] == "stress":
        assert m.counters[3] > 0, "no UB tick"


@pytest.mark.parametrize("case", RC.STREAM_CASES, ids=[c["name"] for c in RC.STREAM_CASES])
def test_stream_schedule_restarts_in_different_calls(oracle, case):
    m = RC.model_of(oracle, case)
    seen_marked = False
    for a, b in RC.stream_schedule(case):
        for i, moves in a + b:
            log = m.tick(*case["ranges"][i], moves)
            seen_marked |= bool(log["marked_outside"])
    for i in range(len(case["ranges"])):
        assert any(c["restarted"] for c in _of_range(case, m, i)), f"range {i} never restarts an env"
    restarting = {j % (len(RC.STREAM_A) + len(RC.STREAM_B)) for j, c in enumerate(m.calls) if c["restarted"]}
    assert len(restarting) >= 4, "the restarts do not fall in different calls of a round"
    assert seen_marked or case["reset"] != RESET_AT_END


def test_observation_schedule_shows_restarted_envs(oracle):
    case = RC.OBS_CASE
    m = RC.model_of(oracle, case)
    marked = 0
    for i, moves in RC.schedule(case, RC.OBS_ROUNDS):
        first, count = case["ranges"][i]
        m.tick(first, count, moves)
        marked += int(m.finished[first:first + count].sum())   # what the call's observation shows as restarted
    assert marked > case["n"] // 2
    assert all(any(c["restarted"] for c in _of_range(case, m, i)) for i in range(len(case["ranges"])))
    assert sum(c["by_deaths"] for c in m.calls) >= 1 and m.counters[1] > sum(c["by_deaths"] for c in m.calls), "ends by deaths and by the bound"


@pytest.mark.parametrize("reset", [RESET_AT_START, RESET_AT_END])
def test_range_ticks_between_chained_calls_restart_somebody(oracle, reset):
    case = RC.chain_case(reset)
    m = RC.model_of(oracle, case)
    m.random_ticks(RC.CHAIN_SEED, DIST_RANDOM, RC.CHAIN_TICK0, RC.CHAIN_TICKS)
    before = len(m.calls)
    for i, moves in RC.chain_range_ticks(case):
        m.tick(*case["ranges"][i], moves)
    assert sum(len(c["restarted"]) for c in m.calls[before:]) >= 3, "the range ticks restart nobody"
    assert sum(len(c["restarted"]) for c in m.calls[:before]) >= 3, "the first chained call restarts nobody"
    # the second chained call tells tick 27 from tick 30: a range tick that advanced the handle's tick would show
    right, wrong = RC.model_of(oracle, case), RC.model_of(oracle, case)
    right.random_ticks(RC.CHAIN_SEED, DIST_RANDOM, RC.CHAIN_TICK0 + RC.CHAIN_TICKS, 2)
    wrong.random_ticks(RC.CHAIN_SEED, DIST_RANDOM, RC.CHAIN_TICK0 + RC.CHAIN_TICKS + 3, 2)
    assert "state" in right.differences(wrong)


# ---- the schedules tell a wrong kernel from a right one -----------------------------------------------------------------------------
class KeyRelativeToTheRange(RangeModel):
    def _board_env(self, e, first):
        return self.env_offset + e - first


class SnapshotRelativeToTheRange(RangeModel):
    def _snapshot_of(self, e, first):
        return self.snapshot[e - first]


class EveryCallClearsEveryMark(RangeModel):
    def _before_call(self, first, count):
        self.finished[:] = 0


class ShortLastTileNotCounted(RangeModel):
    def _count_restart(self, e):
        if e < self.n - self.n % 16:
            self.counters[2] += 1


class RestartsOutsideTheRange(RangeModel):
    def _before_call(self, first, count):
        for e in list(range(first)) + list(range(first + count, self.n)):
            if self.done[e] and self.auto_reset == RESET_AT_START:
                self._restart(e, first, dict(restarted=[]))


WRONG = [  # (variant, the cases it can show in, what must differ at least)
    (KeyRelativeToTheRange, lambda c: c["fresh"] and c["reset"] != RESET_OFF, "state"),
    (SnapshotRelativeToTheRange, lambda c: not c["fresh"] and c["reset"] != RESET_OFF, "state"),
    (EveryCallClearsEveryMark, lambda c: c["reset"] == RESET_AT_END, "last_finished"),
    (ShortLastTileNotCounted, lambda c: c["reset"] != RESET_OFF, "counters"),
    (RestartsOutsideTheRange, lambda c: c["reset"] == RESET_AT_START, "status_done"),
]


@pytest.mark.parametrize("variant,applies,field", WRONG, ids=[w[0].__name__ for w in WRONG])
def test_wrong_variants_are_told_apart(oracle, variant, applies, field):
    """in EVERY case in which the mistake can show it does show, in something same_as compares"""
    cases = [c for c in RC.CASES if applies(c)]
    assert len(cases) >= 2
    for case in cases:
        right, wrong = RC.model_of(oracle, case), RC.model_of(oracle, case, variant)
        first_seen = None
        for j, (i, moves) in enumerate(RC.schedule(case)):
            right.tick(*case["ranges"][i], moves)
            wrong.tick(*case["ranges"][i], moves)
            if first_seen is None and right.differences(wrong):
                first_seen = j, right.differences(wrong)
        assert first_seen is not None, f"{variant.__name__} passes for the model in {case['name']}"
        assert field in first_seen[1] or field in right.differences(wrong), (case["name"], first_seen)
    for case in RC.STREAM_CASES:
        if applies(case):
            right, wrong = RC.model_of(oracle, case), RC.model_of(oracle, case, variant)
            seen = False
            for a, b in RC.stream_schedule(case):
                for i, moves in a + b:
                    right.tick(*case["ranges"][i], moves)
                    wrong.tick(*case["ranges"][i], moves)
                seen |= bool(right.differences(wrong))   # compared where the GPU test compares: after a round
            assert seen, f"{variant.__name__} passes for the model in the stream case {case['name']}"
