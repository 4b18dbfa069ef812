"""Inputs of the forecast tests (pom_batch_forecast, include/pom_batch.h PomForecastSpec) — test infrastructure, numpy only.

hand_made(): small states built by hand, each about one thing a forecast must get right, with the first-tick moves and the horizon
they are forecast with.  What they must give is written out by hand in tests/test_forecast_host.py, not here.
played(): start boards of both kinds played on by the oracle under the random move stream, forecast idle and with random
first-tick moves.  tests/golden/gen_forecast.py runs both through the compiled reference."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import pomcpp_amd as pa
import pomcpp_amd.state as S
from pomcpp_amd.state import Item, Move

I, U, D, L, R, B = Move.IDLE, Move.UP, Move.DOWN, Move.LEFT, Move.RIGHT, Move.BOMB
HORIZONS = (1, 4, 12, 16, 32)


@dataclass
class Case:
    name: str
    start: np.ndarray   # STATE_DTYPE[1]
    moves: object       # None (idle) or the four moves of tick 1
    horizon: int


def _base():
    s = S.new_states(1)
    S.put_agents_in_corners(s[0])   # agent 0 (0, 0), 1 (10, 0), 2 (10, 10), 3 (0, 10)
    return s


def _move_agent(s, agent, x, y):
    a = s["agents"][0, agent]
    s["board"][0, int(a["y"]), int(a["x"])] = Item.PASSAGE
    S.put_agent(s[0], x, y, agent)


def _kill(s, *agents):
    for a in agents:
        ag = s["agents"][0, a]
        s["board"][0, int(ag["y"]), int(ag["x"])] = Item.PASSAGE
    S.kill(s[0], *agents)


def _bomb(s, x, y, owner, life, strength, direction=0):
    s["agents"][0, owner]["bombStrength"] = strength
    s["agents"][0, owner]["maxBombCount"] = 5
    k = int(s["bombs_count"][0])
    S.plant_bomb(s[0], x, y, owner, set_item=True, life_time=life)
    if direction:
        S.set_bomb_direction(s[0], k, direction)


def _flame(s, x, y, time_left, strength=1):
    """a flame as State::SpawnFlame leaves it on an open board: the queue entry and its cross of cells"""
    k = int(s["flames_count"][0])
    s["flames_queue"][0, k] = (x, y, time_left, strength)
    s["flames_count"] = k + 1
    for d in range(-strength, strength + 1):
        for cx, cy in ((x + d, y), (x, y + d)):
            if 0 <= cx <= 10 and 0 <= cy <= 10:
                s["board"][0, cy, cx] = Item.FLAMES + ((x + 11 * y) << 3)


def hand_made():
    out = []
    # a short-fused bomb inside the cross of a long-fused one: the long one goes off with it (the case strategy::IsInDanger gets wrong)
    s = _base()
    _bomb(s, 5, 5, 1, life=2, strength=2)
    _bomb(s, 7, 5, 2, life=8, strength=2)
    out.append(Case("early_chain", s, None, 8))
    # one ray stopped by rigid, one by wood (the wood burns, the cell behind does not)
    s = _base()
    _bomb(s, 5, 5, 0, life=3, strength=3)
    s["board"][0, 5, 7] = Item.RIGID
    s["board"][0, 7, 5] = Item.WOOD
    out.append(Case("blocked_rays", s, None, 4))
    # a kicked bomb on its way: it rolls right for three ticks and goes off where it has got to
    s = _base()
    _bomb(s, 2, 5, 0, life=3, strength=1, direction=S.Direction.RIGHT)
    out.append(Case("moving_bomb", s, None, 5))
    # a flame about to go out (its cells read 0), one of its cells lit again in the very tick it goes out, and a flame that stays
    s = _base()
    _flame(s, 3, 3, time_left=1)
    _flame(s, 8, 8, time_left=3)
    _bomb(s, 3, 5, 0, life=1, strength=1)
    out.append(Case("expiring_flames", s, None, 3))
    # an agent that dies where it stands, and one that was dead before
    s = _base()
    _move_agent(s, 1, 5, 6)
    _kill(s, 3)
    _bomb(s, 5, 5, 0, life=4, strength=1)
    out.append(Case("agent_deaths", s, None, 6))
    # a finished game (one agent alive) is forecast like any other
    s = _base()
    _kill(s, 1, 2, 3)
    _bomb(s, 5, 5, 0, life=2, strength=1)
    out.append(Case("finished_game", s, None, 3))
    # first-tick moves.  BOMB: planted with BOMB_LIFETIME + 1 and ticked in the same Step (step.cpp:54), it goes off on tick 11 under
    # the agent that stays on it
    out.append(Case("move_bomb", _base(), (B, I, I, I), 12))
    out.append(Case("move_bomb_horizon32", _base(), (B, I, I, I), 32))
    # stepping out of a cross that goes off on tick 1: the agent survives (idle it would not: the same state without the move)
    s = _base()
    _move_agent(s, 0, 5, 5)
    _bomb(s, 3, 5, 1, life=1, strength=2)
    out.append(Case("step_out", s, (D, I, I, I), 2))
    out.append(Case("stay_in", s.copy(), None, 2))
    # stepping into flames (step.cpp:84-98), horizon 1
    s = _base()
    _move_agent(s, 0, 7, 5)
    _flame(s, 5, 5, time_left=3)
    out.append(Case("step_into_flames", s, (L, I, I, I), 1))
    for c in out:
        c.start["agents"]["pad"] = 0
    return out


def played_states(oracle, kind, n, ticks, seed=3):
    """n start boards of a kind played on for `ticks` ticks by the oracle under the random move stream (as tests/test_observe_view.py)"""
    start = pa.make_boards(n, seed=seed, kind=kind)
    states = start.copy()
    oracle.run_random(states, start, ticks, seed, 0, 0, 2 if kind == "stress" else 1, 300)
    states["agents"]["pad"] = 0
    return states


def random_moves(n, seed):
    return np.random.default_rng(seed).integers(0, 6, size=(n, 4), dtype=np.int32)


def played(oracle, per_kind=24):
    """the fixture's played entries: (kind, ticks) x (idle, random first moves), the horizons in rotation"""
    out = []
    for kind, ticks in (("ffa", 57), ("stress", 23)):
        states = played_states(oracle, kind, per_kind, ticks)
        mv = random_moves(per_kind, 7 + ticks)
        for with_moves in (False, True):
            for e in range(per_kind):
                out.append(Case(f"{kind}{ticks}_{'mv' if with_moves else 'idle'}_{e}", states[e:e + 1].copy(),
                                tuple(int(v) for v in mv[e]) if with_moves else None, HORIZONS[(e + with_moves) % len(HORIZONS)]))
    return out


def all_cases(oracle):
    return hand_made() + played(oracle)
