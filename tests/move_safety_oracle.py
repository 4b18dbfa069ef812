"""TEST INFRASTRUCTURE — the checker of pom_batch_move_safety (include/pom_batch.h PomMoveSafetySpec): for every live agent and each
of its six candidate moves a copy of the state is played K ticks by Oracle.step (tick 1 with the candidate in the agent's entry, then
IDLE), recording the tick the agent dies in and the tick the walker's set R runs empty.  Nothing of the kernel's own logic is restated
here: the tick is the oracle's, Free is read off the State's board values, and R is a boolean [11, 11] array per play grown by four
slice assignments — no 121-bit words, no shifts, no masks.  All plays advance together, a tick at a time, so that numpy does the sets."""
import numpy as np

from pomcpp_amd.state import Item

UNASKED = -7   # the rows of agents that were not asked for: a value no answer has


def free_cells(board: np.ndarray) -> np.ndarray:
    """bool [..., 11, 11]: PASSAGE or IS_POWERUP (bboard.hpp:77-84)"""
    return (board == Item.PASSAGE) | ((board > 5) & (board < 9))


def grow(reach: np.ndarray, free: np.ndarray) -> np.ndarray:
    """R_t from R_{t-1}: the set and its four neighbours on the board, cut to the free cells; bool [..., 11, 11], row-major [y][x]"""
    g = reach.copy()
    g[..., 1:, :] |= reach[..., :-1, :]
    g[..., :-1, :] |= reach[..., 1:, :]
    g[..., :, 1:] |= reach[..., :, :-1]
    g[..., :, :-1] |= reach[..., :, 1:]
    return g & free


def at_horizon(ticks: np.ndarray, horizon: int) -> np.ndarray:
    """the answers for a shorter horizon from those of a longer one: the shorter play is a prefix of the longer, so what happens
    after its last tick has not happened"""
    return np.where(ticks > horizon, 0, ticks).astype(np.int8)


def move_safety(oracle, states: np.ndarray, horizon: int, moves=None, agents=(0, 1, 2, 3), step=None):
    """states STATE_DTYPE[n] (not changed), moves int32[n, 4] (the others' moves of tick 1) or None -> death_tick, escape_tick
    int8[n, 4, 6]; the rows of agents not in `agents` are UNASKED.  `step(state, moves)` replaces the oracle's step (the fixture's
    generator plays the compiled reference)."""
    n = states.size
    step = step or oracle.step
    death = np.full((n, 4, 6), UNASKED, dtype=np.int8)
    escape = np.full((n, 4, 6), UNASKED, dtype=np.int8)
    agents = list(agents)
    death[:, agents], escape[:, agents] = -1, -1
    # one play per (env, live agent asked for, candidate)
    env, who = np.nonzero(states["agents"]["dead"][:, agents] == 0)
    who = np.asarray(agents)[who]
    env, who, cand = np.repeat(env, 6), np.repeat(who, 6), np.tile(np.arange(6), env.size)
    V = env.size
    play = states[env].copy()
    first = np.zeros((V, 4), dtype=np.int32) if moves is None else np.ascontiguousarray(moves, dtype=np.int32)[env].copy()
    first[np.arange(V), who] = cand
    idle = np.zeros(4, dtype=np.int32)
    d, x = np.zeros(V, dtype=np.int8), np.zeros(V, dtype=np.int8)
    reach = np.zeros((V, 11, 11), dtype=bool)
    v = np.arange(V)
    for t in range(1, horizon + 1):
        for i in range(V):
            step(play[i:i + 1], first[i] if t == 1 else idle)
        me = play["agents"][v, who]
        alive = me["dead"] == 0
        d[(d == 0) & ~alive] = t
        own = np.zeros((V, 11, 11), dtype=bool)
        own[v[alive], me["y"][alive], me["x"][alive]] = True
        reach = own if t == 1 else grow(reach, free_cells(play["board"]) | own)
        x[(x == 0) & ~reach.any(axis=(1, 2))] = t
    death[env, who, cand], escape[env, who, cand] = d, x
    return death, escape
