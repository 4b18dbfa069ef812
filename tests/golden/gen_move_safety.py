#!/usr/bin/env python3
"""Generate tests/golden/move_safety.npz: what pom_batch_move_safety (include/pom_batch.h PomMoveSafetySpec) must give on the cases of
tests/move_safety_cases.py, played by the COMPILED, UNMODIFIED reference (oracle/_ref/libpomref.so, ref_step).

Runs in the build container only, like gen_forecast.py.  For every case: its start state, the others' moves of tick 1, the horizon,
and the two outputs for all four agents — the states are the reference's, the sets on top of them tests/move_safety_oracle.py's.  No
play raises one of the reference's crashing UBs (asserted with the oracle before every tick: pick another seed, do not filter), so the
reference plays every tick of every candidate.

  names str[A]   start uint8[A, 1004]   has_moves uint8[A]   moves int32[A, 4]   horizon int32[A]
  death_tick int8[A, 4, 6]   escape_tick int8[A, 4, 6]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.case_api import RefAPI  # noqa: E402
from tests.edge_states import FATAL  # noqa: E402
from tests.move_safety_cases import all_cases  # noqa: E402
from tests.move_safety_oracle import move_safety  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "move_safety.npz")


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

    death = np.zeros((A, 4, 6), dtype=np.int8)
    escape = np.zeros((A, 4, 6), dtype=np.int8)
    moves = np.zeros((A, 4), dtype=np.int32)
    for i, c in enumerate(cases):
        name[0] = c.name
        if c.moves is not None:
            moves[i] = c.moves
        d, x = move_safety(oracle, c.start, c.horizon, None if c.moves is None else moves[i:i + 1], step=ref_step)
        death[i], escape[i] = d[0], x[0]
    np.savez_compressed(
        OUT,
        names=np.array([c.name for c in cases]),
        start=np.frombuffer(b"".join(c.start.tobytes() for c in cases), dtype=np.uint8).reshape(A, 1004),
        has_moves=np.array([c.moves is not None for c in cases], dtype=np.uint8), moves=moves,
        horizon=np.array([c.horizon for c in cases], dtype=np.int32), death_tick=death, escape_tick=escape,
    )
    print(f"move_safety.npz: {A} cases, {int((death > 0).sum())} fatal candidates, {int((escape > 0).sum())} without a way out, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
