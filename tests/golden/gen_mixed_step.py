#!/usr/bin/env python3
"""Generate tests/golden/mixed_step.npz: what pom_batch_step_mixed (include/pom_batch.h PomMixedStepSpec) must leave, whole batch,
POM_RESET_AT_START from the snapshot, every tick played by the COMPILED, UNMODIFIED reference (oracle/_ref/libpomref.so, ref_step) and
every act() by its agents::SimpleAgent (ref_simple_act).

Runs in the build container only, like gen_rollout_policy.py, whose method this is: an agent is a reference SimpleAgent whose memory is
set (ref_simple_set_memory) to what the game carries and whose generator is reseeded until the draw it is about to make
(ref_simple_peek_draw) is the stream's.  The loop around them is the header's six steps written out: a finished env restarts from its
start state with zero memory for all four agents; the LIVE agents of the mask are asked, the others take the tape's moves (dead agents'
entries included); Step; timeStep++ and the done rule of environment.cpp:148-168 with the max_steps bound.  No tick raises one of the
reference's crashing UBs (asserted with the checker before every tick: pick another seed, do not filter).

  start uint8[N, 1004]  moves int32[T, N, 4]  states uint8[T, N, 1004]  mems int32[T, N, 4, 16]   (states / mems: after tick t)
  mask seed tick0 env_offset max_steps restarts dead_in_mask: scalars
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests.edge_states import FATAL  # noqa: E402
from tests.golden.gen_rollout_policy import ref_lib  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402
from tests.test_visit_path import burned_in  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mixed_step.npz")
N, T, MASK, SEED, TICK0, ENV_OFFSET, MAX_STEPS, BOARD_SEED = 40, 30, 0b1010, 2024, (1 << 32) - 30, 700, 52, 19   # the last tick is 2^32 - 1


def main():
    ref, oracle = ref_lib(), Oracle()
    oracle.lib.pom_oracle_policy_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    seed_for = {}   # (agent, draw) -> a generator seed whose first draw is that value

    def agent_with_draw(a, want):
        k = seed_for.get((a, want), 1)
        while True:
            obj = C.c_void_p(ref.ref_simple_new(a, k))
            if ref.ref_simple_peek_draw(obj) == want:
                seed_for[(a, want)] = k
                return obj
            ref.ref_simple_delete(obj)
            k += 1

    start = burned_in(oracle, N, BOARD_SEED)   # games of every age, dead agents among them, none finished
    S, M, done = start.copy(), np.zeros((N, 4, 16), dtype=np.int32), np.zeros(N, dtype=bool)
    tape = np.random.default_rng(5).integers(0, 6, size=(T, N, 4), dtype=np.int32)
    states, mems = np.zeros((T, N, 1004), dtype=np.uint8), np.zeros((T, N, 4, 16), dtype=np.int32)
    restarts = dead_in_mask = acts = 0
    for t in range(T):
        for e in range(N):
            if done[e]:   # 1: restart at the start, fresh agents, all four
                S[e], M[e], done[e] = start[e], 0, False
                restarts += 1
            mv = tape[t, e].copy()
            for a in range(4):
                if not MASK >> a & 1:
                    continue   # 4: the caller's move, dead agents' included
                if S["agents"]["dead"][e, a]:
                    mv[a] = 0   # 3: a dead agent of the mask gives IDLE
                    dead_in_mask += 1
                    continue
                obj = agent_with_draw(a, int(oracle.lib.pom_oracle_policy_draw(SEED, ENV_OFFSET + e, (TICK0 + t) & 0xFFFFFFFF, a)))
                mem = np.ascontiguousarray(M[e, a])
                ref.ref_simple_set_memory(obj, mem.ctypes.data)
                mv[a] = ref.ref_simple_act(obj, S[e:e + 1].ctypes.data)
                ref.ref_simple_memory(obj, mem.ctypes.data)
                M[e, a] = mem
                ref.ref_simple_delete(obj)
                acts += 1
            probe = S[e:e + 1].copy()
            assert not oracle.step(probe, mv) & FATAL, (t, e)
            ref.ref_step(S[e:e + 1].ctypes.data, mv.ctypes.data)   # 5: the tick
            S["timeStep"][e] += 1
            done[e] = S["aliveAgents"][e] <= 1 or S["timeStep"][e] >= MAX_STEPS
        S["agents"]["pad"] = 0
        states[t] = np.frombuffer(S.tobytes(), dtype=np.uint8).reshape(N, 1004)
        mems[t] = M
    assert restarts >= N // 2 and dead_in_mask > 0, (restarts, dead_in_mask)
    assert TICK0 + T - 1 < 1 << 32
    np.savez_compressed(OUT, start=np.frombuffer(start.tobytes(), dtype=np.uint8).reshape(N, 1004), moves=tape, states=states, mems=mems,
                        mask=np.int32(MASK), seed=np.int64(SEED), tick0=np.int64(TICK0), env_offset=np.int64(ENV_OFFSET),
                        max_steps=np.int32(MAX_STEPS), restarts=np.int64(restarts), dead_in_mask=np.int64(dead_in_mask))
    print(f"mixed_step.npz: {N} envs x {T} ticks, mask {MASK:#x}, {acts} reference act() calls, {restarts} restarts, "
          f"{dead_in_mask} dead agents of the mask passed over; {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
