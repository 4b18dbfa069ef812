#!/usr/bin/env python3
"""Generate tests/golden/forecast.npz: what pom_batch_forecast (include/pom_batch.h PomForecastSpec) must give on the cases of
tests/forecast_cases.py, played by the COMPILED, UNMODIFIED reference (oracle/_ref/libpomref.so, ref_step).

Runs in the build container only, like gen_tile_mates.py.  For every case: its start state, the moves of tick 1, the horizon, and the
two outputs the reference's states define — per cell the first tick that leaves it in flames, per agent the tick it dies in.  No case
raises one of the reference's crashing UBs (asserted with the oracle before every tick: pick another seed, do not filter), so the
reference plays every tick of every case.

  names str[A]   start uint8[A, 1004]   has_moves uint8[A]   moves int32[A, 4]   horizon int32[A]
  flame_tick uint8[A, 11, 11]   agent_tick int32[A, 4]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.case_api import RefAPI  # noqa: E402
from tests.edge_states import FATAL  # noqa: E402
from tests.forecast_cases import all_cases  # noqa: E402
from tests.forecast_oracle import forecast  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "forecast.npz")


def main():
    ref = RefAPI().lib
    oracle = Oracle()
    cases = all_cases(oracle)
    A = len(cases)
    name = [""]

    def ref_step(s, mv):
        mv = np.ascontiguousarray(mv, dtype=np.int32)
        probe = s.copy()
        assert not oracle.step(probe, mv) & FATAL, name[0]
        ref.ref_step(s.ctypes.data, mv.ctypes.data)
        return 0

    flame = np.zeros((A, 11, 11), dtype=np.uint8)
    agent = np.zeros((A, 4), dtype=np.int32)
    moves = np.zeros((A, 4), dtype=np.int32)
    for i, c in enumerate(cases):
        name[0] = c.name
        if c.moves is not None:
            moves[i] = c.moves
        f, a, _ = forecast(oracle, c.start, c.horizon, None if c.moves is None else moves[i:i + 1], step=ref_step)
        flame[i], agent[i] = f[0], a[0]
    np.savez_compressed(
        OUT,
        names=np.array([c.name for c in cases]),
        start=np.frombuffer(b"".join(c.start.tobytes() for c in cases), dtype=np.uint8).reshape(A, 1004),
        has_moves=np.array([c.moves is not None for c in cases], dtype=np.uint8), moves=moves,
        horizon=np.array([c.horizon for c in cases], dtype=np.int32), flame_tick=flame, agent_tick=agent,
    )
    print(f"forecast.npz: {A} cases, {int((flame > 0).sum())} cells in flames, {int((agent > 0).sum())} deaths, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
