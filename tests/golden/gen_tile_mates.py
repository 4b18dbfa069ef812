#!/usr/bin/env python3
"""Generate tests/golden/tile_mates.npz: the actors of tests/tile_mates.py stepped by the COMPILED, UNMODIFIED reference
(oracle/_ref/libpomref.so).

Runs in the build container only, like gen_edge_cases.py.  For every actor: its start state and Move[4] script, the blake2b-64 of
the reference's state after every tick, and full states after ticks 1, 2, 8 and the last.  No actor raises one of the reference's
crashing UBs (checked with the oracle before every tick), so the reference plays every tick of every script.

  names   str[A]   start  uint8[A, 1004]   moves  int32[A, T, 4]   hashes  uint64[A, T]
  ck_entry / ck_tick int32[C], ck_state uint8[C, 1004]   (ck_tick = ticks played so far)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.case_api import RefAPI  # noqa: E402
from tests.edge_states import FATAL  # noqa: E402
from tests.golden.gen_golden import state_hash  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402
from tests.tile_mates import TICKS, actors  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "tile_mates.npz")
CK_TICKS = (1, 2, 8, TICKS)


def main():
    ref = RefAPI().lib
    oracle = Oracle()
    entries = actors(oracle)
    A = len(entries)
    hashes = np.zeros((A, TICKS), dtype=np.uint64)
    ck_entry, ck_tick, ck_state = [], [], []
    for i, e in enumerate(entries):
        s = e.start.copy()
        for t, mv in enumerate(e.moves):
            probe = s.copy()
            assert not oracle.step(probe, mv) & FATAL, (e.name, t)
            ref.ref_step(s.ctypes.data, np.ascontiguousarray(mv, dtype=np.int32).ctypes.data)
            s["agents"]["pad"] = 0
            hashes[i, t] = state_hash(s.tobytes())
            if t + 1 in CK_TICKS:
                ck_entry.append(i)
                ck_tick.append(t + 1)
                ck_state.append(s.tobytes())
    np.savez_compressed(
        OUT,
        names=np.array([e.name for e in entries]),
        start=np.frombuffer(b"".join(e.start.tobytes() for e in entries), dtype=np.uint8).reshape(A, 1004),
        moves=np.stack([e.moves for e in entries]).astype(np.int32), hashes=hashes,
        ck_entry=np.array(ck_entry, dtype=np.int32), ck_tick=np.array(ck_tick, dtype=np.int32),
        ck_state=np.frombuffer(b"".join(ck_state), dtype=np.uint8).reshape(-1, 1004),
    )
    print(f"tile_mates.npz: {A} actors x {TICKS} reference ticks, {len(ck_state)} full states, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
