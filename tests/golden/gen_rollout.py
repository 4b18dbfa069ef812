#!/usr/bin/env python3
"""Generate tests/golden/rollout.npz: what pom_batch_rollout (include/pom_batch.h PomRolloutSpec) must give on the cases of
tests/rollout_cases.py, every tick played by the COMPILED, UNMODIFIED reference (oracle/_ref/libpomref.so, ref_step).

Runs in the build container only, like gen_forecast.py.  The loop around the tick — the pom_rng.h move stream, timeStep++, the
done / winner / draw rule, the result word — is the checker's (tests/rollout_oracle.py) with the reference's Step put in.  No tick of any
case raises one of the reference's crashing UBs (asserted with the oracle before every tick: pick another seed, do not filter).

  names str[G]  kind int32[G]  horizon int32[G]  has_moves uint8[G]  result uint32[G, samples, 24]
  states uint8[2, 24, 1004]  moves int32[2, 24, 4]  dist int32[2]  seed int64  samples int32
  hand_names str[H]  hand_pre uint8[H, 1004]  hand_pre_ticks / hand_max_steps / hand_horizon int32[H]
  hand_start uint8[H, 1004]  hand_start_word uint32[H]  hand_result uint32[H, samples]
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import rollout_cases as RC  # noqa: E402
from tests import rollout_oracle as RO  # noqa: E402
from tests.case_api import RefAPI  # noqa: E402
from tests.edge_states import FATAL  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rollout.npz")
OUTCOME = RO.RO_DONE | RO.RO_DRAW | RO.RO_TIMEOUT | 7 << RO.RO_WINNER_SHIFT


def main():
    ref = RefAPI().lib
    oracle = Oracle()
    name, last = [""], [None]

    def ref_step(s, mv):
        mv = np.ascontiguousarray(mv, dtype=np.int32)
        probe = s.copy()
        assert not oracle.step(probe, mv) & FATAL, name[0]
        ref.ref_step(s.ctypes.data, mv.ctypes.data)
        last[0] = s
        return 0

    states = [RC.kind_states(oracle, i) for i in range(len(RC.KINDS))]
    moves = [RC.kind_moves(i) for i in range(len(RC.KINDS))]
    gs = RC.groups()
    result = np.zeros((len(gs), RC.SAMPLES, RC.PER_KIND), dtype=np.uint32)
    for g, grp in enumerate(gs):
        name[0] = grp.name
        result[g] = RO.rollout(oracle, states[grp.kind], grp.horizon, RC.SAMPLES, RC.SEED, RC.KINDS[grp.kind][2],
                               moves[grp.kind] if grp.with_moves else None, step=ref_step)
    # the fixture as a whole is not one-sided (another seed if it is; nothing is filtered)
    length, k = result >> RO.RO_LENGTH_SHIFT, np.array([grp.horizon for grp in gs])[:, None, None]
    early, full = int(((result & RO.RO_DONE != 0) & (length < k)).sum()), int((length == k).sum())
    winners, draws = int((result >> RO.RO_WINNER_SHIFT & 7 != 0).sum()), int((result & RO.RO_DRAW != 0).sum())
    assert 4 * early >= result.size and 4 * full >= result.size and winners >= 10 and draws >= 1, (early, full, winners, draws, result.size)
    assert not (result & RO.RO_UB).any()

    hands = RC.hand_made()
    H = len(hands)
    hand_start = np.zeros((H, 1004), dtype=np.uint8)
    hand_word = np.zeros(H, dtype=np.uint32)
    hand_result = np.zeros((H, RC.SAMPLES), dtype=np.uint32)
    for i, h in enumerate(hands):
        name[0] = h.name
        start, word = h.pre, 0
        if h.pre_ticks:   # the all-IDLE ticks that lead to S_0, with the same bookkeeping
            assert h.pre_ticks == 1
            word = int(RO.rollout(oracle, h.pre, 1, 1, 0, RO.DIST_RANDOM, np.zeros((1, 4), dtype=np.int32), h.max_steps, step=ref_step)[0, 0]) & OUTCOME
            start = last[0].copy()
        hand_start[i], hand_word[i] = np.frombuffer(start.tobytes(), dtype=np.uint8), word
        hand_result[i] = RO.rollout(oracle, start, h.horizon, RC.SAMPLES, RC.SEED, RO.DIST_RANDOM, None, h.max_steps,
                                    start=np.array([word], dtype=np.uint32), step=ref_step)[:, 0]
    np.savez_compressed(
        OUT,
        names=np.array([grp.name for grp in gs]), kind=np.array([grp.kind for grp in gs], dtype=np.int32),
        horizon=np.array([grp.horizon for grp in gs], dtype=np.int32), has_moves=np.array([grp.with_moves for grp in gs], dtype=np.uint8),
        result=result,
        states=np.stack([np.frombuffer(s.tobytes(), dtype=np.uint8).reshape(RC.PER_KIND, 1004) for s in states]),
        moves=np.stack(moves).astype(np.int32), dist=np.array([k[2] for k in RC.KINDS], dtype=np.int32),
        seed=np.int64(RC.SEED), samples=np.int32(RC.SAMPLES),
        hand_names=np.array([h.name for h in hands]),
        hand_pre=np.stack([np.frombuffer(h.pre.tobytes(), dtype=np.uint8) for h in hands]),
        hand_pre_ticks=np.array([h.pre_ticks for h in hands], dtype=np.int32),
        hand_max_steps=np.array([h.max_steps for h in hands], dtype=np.int32),
        hand_horizon=np.array([h.horizon for h in hands], dtype=np.int32),
        hand_start=hand_start, hand_start_word=hand_word, hand_result=hand_result,
    )
    print(f"rollout.npz: {len(gs)} groups of {RC.SAMPLES} x {RC.PER_KIND} playouts: {early} finish early, {full} play all K ticks, "
          f"{winners} winners, {draws} draws; {H} hand-made; {os.path.getsize(OUT)} bytes")
    print("hand-made words:", {h.name: [hex(int(w)) for w in hand_result[i]] for i, h in enumerate(hands)})


if __name__ == "__main__":
    main()
