#!/usr/bin/env python3
"""Generate tests/golden/edge_cases.npz: the record-edge corpus (tests/edge_states.py) stepped by the COMPILED, UNMODIFIED
reference (oracle/_ref/libpomref.so).

Runs in the build container only, like gen_golden.py.  For every entry: its start state and Move[4] script, the blake2b-64 of
the reference's state after every tick, and full states every 32 ticks and after the last tick.  As in gen_golden.py the
reference is never stepped on a tick for which the oracle predicts one of its crashing UBs (NULL_BOMB, QUEUE_OVERFLOW,
REVERT_LOOP, BAD_INDEX): the entry's trace ends before it.

  start   uint8[E, 1004]     moves   int32[M, 4]   (entry e's script: moves[moff[e]:moff[e+1]])
  names   str[E]             hashes  uint64[H]     (entry e's ticks played: hoff[e+1] - hoff[e] <= its script's length)
  ck_entry / ck_tick int32[C], ck_state uint8[C, 1004]   (ck_tick = ticks played so far)
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.case_api import RefAPI  # noqa: E402
from tests.edge_states import FATAL, corpus  # noqa: E402
from tests.golden.gen_golden import state_hash  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "edge_cases.npz")
CK_EVERY = 32


def main():
    ref = RefAPI().lib
    oracle = Oracle()
    entries = corpus(oracle)
    starts, moves, moff, hashes, hoff, ck_entry, ck_tick, ck_state = [], [], [0], [], [0], [], [], []
    for e_i, e in enumerate(entries):
        s = e.start.copy()
        starts.append(s.tobytes())
        moves.append(e.moves)
        moff.append(moff[-1] + len(e.moves))
        n = 0
        for mv in e.moves:
            probe = s.copy()
            if oracle.step(probe, mv) & FATAL:
                break
            ref.ref_step(s.ctypes.data, np.ascontiguousarray(mv, dtype=np.int32).ctypes.data)
            s["agents"]["pad"] = 0
            hashes.append(state_hash(s.tobytes()))
            n += 1
            if n % CK_EVERY == 0 or n == len(e.moves):
                ck_entry.append(e_i)
                ck_tick.append(n)
                ck_state.append(s.tobytes())
        if n < len(e.moves) and (not ck_tick or ck_entry[-1] != e_i or ck_tick[-1] != n):
            ck_entry.append(e_i)  # the state before the tick the reference was not given
            ck_tick.append(n)
            ck_state.append(s.tobytes())
        hoff.append(hoff[-1] + n)
        print(f"  {e.name}: {n} of {len(e.moves)} ticks, flames.count {int(s['flames_count'][0])}")
    E = len(entries)
    np.savez_compressed(
        OUT,
        names=np.array([e.name for e in entries]),
        start=np.frombuffer(b"".join(starts), dtype=np.uint8).reshape(E, 1004),
        moves=np.concatenate(moves).astype(np.int32), moff=np.array(moff, dtype=np.int64),
        hashes=np.array(hashes, dtype=np.uint64), hoff=np.array(hoff, dtype=np.int64),
        ck_entry=np.array(ck_entry, dtype=np.int32), ck_tick=np.array(ck_tick, dtype=np.int32),
        ck_state=np.frombuffer(b"".join(ck_state), dtype=np.uint8).reshape(-1, 1004),
    )
    print(f"edge_cases.npz: {E} entries, {hoff[-1]} reference ticks of {moff[-1]}, {len(ck_state)} full states, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
