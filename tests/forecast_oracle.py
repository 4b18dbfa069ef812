"""TEST INFRASTRUCTURE — the checker of pom_batch_forecast (include/pom_batch.h PomForecastSpec): K x Oracle.step on a copy of
every state, recording per cell the first tick that leaves it in flames, per agent the tick it dies in, and the OR of the ticks'
POM_UB_* flags.  Nothing of the kernel's own logic is restated here: the tick is the oracle's, the rest is three comparisons."""
import numpy as np

from pomcpp_amd.state import is_flame

IDLE4 = np.zeros(4, dtype=np.int32)


def forecast(oracle, states: np.ndarray, horizon: int, moves=None, step=None):
    """states STATE_DTYPE[n] (not changed), moves int32[n, 4] of tick 1 or None -> flame_tick uint8[n, 11, 11], agent_tick int32[n, 4],
    ubflags uint32[n].  `step(state, moves) -> flags` replaces the oracle's step (the fixture's generator plays the compiled reference)."""
    n = states.size
    step = step or oracle.step
    flame = np.zeros((n, 11, 11), dtype=np.uint8)
    agent = np.zeros((n, 4), dtype=np.int32)
    ub = np.zeros(n, dtype=np.uint32)
    for e in range(n):
        s = states[e:e + 1].copy()
        agent[e] = np.where(s["agents"][0]["dead"] != 0, -1, 0)
        for t in range(1, horizon + 1):
            ub[e] |= np.uint32(step(s, IDLE4 if t > 1 or moves is None else moves[e]))
            burning = is_flame(s["board"][0])   # IS_FLAME, bboard.hpp:85
            flame[e][burning & (flame[e] == 0)] = t
            agent[e][(agent[e] == 0) & (s["agents"][0]["dead"] != 0)] = t
    return flame, agent, ub
