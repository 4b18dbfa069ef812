"""Inputs of the rollout tests (pom_batch_rollout, include/pom_batch.h PomRolloutSpec) — test infrastructure, numpy only.

groups(): the fixture's played entries — the boards of tests/forecast_cases.played_states, each kind under its own move stream,
rolled out at three horizons, with and without first-tick moves.  hand_made(): two states built by hand; what they must give is
written out by hand in tests/test_rollout_host.py, not here.  tests/golden/gen_rollout.py runs both through the compiled reference."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import forecast_cases as FC
from tests.rollout_oracle import DIST_RANDOM, DIST_STRESS

SEED, SAMPLES, PER_KIND = 1236, 4, 24   # (1234 and 1235 raise POM_UB_NULL_BOMB on the 24 stress boards: the reference cannot play those ticks)
HORIZONS = (1, 8, 48)
KINDS = (("ffa", 57, DIST_RANDOM), ("stress", 23, DIST_STRESS))


@dataclass
class Group:
    name: str
    kind: int          # index into KINDS
    horizon: int
    with_moves: bool


def groups():
    return [Group(f"{kind}{ticks}_K{k}_{'mv' if mv else 'rnd'}", i, k, mv)
            for i, (kind, ticks, _) in enumerate(KINDS) for k in HORIZONS for mv in (False, True)]


def kind_states(oracle, i, n=PER_KIND):
    kind, ticks, _ = KINDS[i]
    return FC.played_states(oracle, kind, n, ticks)


def kind_moves(i, n=PER_KIND):
    return FC.random_moves(n, 31 + KINDS[i][1])


@dataclass
class Hand:
    name: str
    pre: np.ndarray     # STATE_DTYPE[1]: uploaded to an ENV-mode handle ...
    pre_ticks: int      # ... and stepped this many all-IDLE ticks: the rollout's S_0
    max_steps: int
    horizon: int


def hand_made():
    out = []
    # agents 2 and 3 are dead, agent 1 stands in the cross of a bomb that goes off in the next tick: one IDLE tick finishes the game
    # with agent 0 the winner, and the rollout finds it finished
    s = FC._base()
    FC._kill(s, 2, 3)
    FC._move_agent(s, 1, 5, 6)
    FC._bomb(s, 5, 5, 0, life=1, strength=1)
    out.append(Hand("finished_game", s, 1, 0, 8))
    # four agents in the corners of an empty board, timeStep 3 short of max_steps: whatever they do, a bomb planted now goes off in
    # tick 10 at the earliest — three ticks are played and the game times out with everybody alive
    s = FC._base()
    s["timeStep"] = 37
    out.append(Hand("three_ticks_left", s, 0, 40, 8))
    for h in out:
        h.pre["agents"]["pad"] = 0
    return out
