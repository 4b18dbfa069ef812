"""Inputs of the move-safety tests (pom_batch_move_safety, include/pom_batch.h PomMoveSafetySpec) — test infrastructure, numpy only.

hand_made(): small states built by hand, each about one thing the two answers must get right, with the others' first-tick moves and
the horizon.  What they must give is written out by hand in tests/test_move_safety_host.py, not here.
played(): start boards of both kinds played on by the oracle under the random move stream (tests/forecast_cases.py), judged with the
others idle and with random first-tick moves.  tests/golden/gen_move_safety.py runs both through the compiled reference."""
from __future__ import annotations

from pomcpp_amd.state import Item
from tests import forecast_cases as FC
from tests.forecast_cases import B, Case, D, I, L, R, U  # noqa: F401  (the moves, for the readers of the rows)

HORIZONS = (1, 4, 12, 32)


def _corner(rigid=(), strength=1):
    """agent 0 in the corner (0, 0) of an empty board, the cells of `rigid` walled"""
    s = FC._base()
    for x, y in rigid:
        s["board"][0, y, x] = Item.RIGID
    s["agents"][0, 0]["bombStrength"] = strength
    return s


def hand_made():
    out = []
    forecast = {c.name: c for c in FC.hand_made()}
    # the move the six-forecast recipe gets wrong: the planted bomb goes off under the agent that stands still in tick 11, but the
    # board is open and a walker is long gone
    out.append(Case("open_corner", _corner(), None, 12))
    # the same corner walled in: nowhere to go, the walker's set is the one cell until the bomb takes it
    out.append(Case("closed_corner", _corner(rigid=((1, 0), (0, 1))), None, 12))
    # a corridor of two cells and a strength-2 bomb: every cell the walker can reach lies in the cross ...
    out.append(Case("corridor_too_short", _corner(rigid=((0, 1), (1, 1), (2, 1), (3, 0)), strength=2), None, 12))
    # ... a third cell, (3, 0), lies outside it
    out.append(Case("corridor_long_enough", _corner(rigid=((0, 1), (1, 1), (2, 1), (3, 1), (4, 0)), strength=2), None, 12))
    # somebody else's bomb about to go off: standing still and stepping along the cross die in tick 3, stepping out of it does not;
    # whoever stands still has had two ticks to walk
    s = FC._base()
    FC._move_agent(s, 0, 5, 5)
    FC._bomb(s, 3, 5, 1, life=3, strength=2)
    out.append(Case("bomb_nearby", s, None, 6))
    # the forecast's pair: the cross goes off in tick 1, only a step out of it survives (the candidate replaces agent 0's entry, so
    # the two give the same rows)
    out.append(Case("step_out", forecast["step_out"].start.copy(), forecast["step_out"].moves, 2))
    out.append(Case("stay_in", forecast["stay_in"].start.copy(), None, 2))
    out.append(Case("step_into_flames", forecast["step_into_flames"].start.copy(), None, 1))
    # an agent that is dead already: six times -1 in both outputs
    s = FC._base()
    FC._kill(s, 3)
    out.append(Case("dead_agent", s, None, 6))
    # another agent's base move takes the cell the candidate wants: agent 0 on (4, 5) is in the cross of a bomb that goes off in tick
    # 1, (5, 5) is outside it — but agent 1 comes from (6, 5) for the same cell and both stay where they are (HasDPCollision, step.cpp:100-103)
    s = FC._base()
    FC._move_agent(s, 0, 4, 5)
    FC._move_agent(s, 1, 6, 5)
    FC._bomb(s, 4, 3, 2, life=1, strength=2)
    out.append(Case("contested_cell", s, (I, L, I, I), 2))
    out.append(Case("uncontested_cell", s.copy(), None, 2))
    for c in out:
        c.start["agents"]["pad"] = 0
    return out


def played(oracle, per_kind=12):
    """the fixture's played entries: (kind, ticks) x (the others idle, random first moves), the horizons in rotation"""
    out = []
    for kind, ticks in (("ffa", 57), ("stress", 23)):
        states = FC.played_states(oracle, kind, per_kind, ticks)
        mv = FC.random_moves(per_kind, 7 + ticks)
        for with_moves in (False, True):
            for e in range(per_kind):
                out.append(Case(f"{kind}{ticks}_{'mv' if with_moves else 'idle'}_{e}", states[e:e + 1].copy(),
                                tuple(int(v) for v in mv[e]) if with_moves else None, HORIZONS[(e + with_moves) % len(HORIZONS)]))
    return out


def all_cases(oracle):
    return hand_made() + played(oracle)
