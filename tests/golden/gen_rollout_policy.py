#!/usr/bin/env python3
"""Generate tests/golden/rollout_policy.npz: what pom_batch_rollout_policy (include/pom_batch.h PomRolloutPolicySpec) must give on the
cases of tests/rollout_policy_cases.py, every tick played by the COMPILED, UNMODIFIED reference (oracle/_ref/libpomref.so, ref_step)
and every act() by its agents::SimpleAgent (ref_simple_act).

Runs in the build container only, like gen_rollout.py.  The loop around them — the pom_rng.h stream, the masks, timeStep++, the done /
winner / draw rule, the result word — is the checker's (tests/rollout_policy_oracle.py) with the reference's Step and act() put in.  An
agent is a reference SimpleAgent whose memory is set (ref_simple_set_memory) to what the playout carries and whose generator is
reseeded until the draw it is about to make (ref_simple_peek_draw) is the stream's: the method of gen_policy_traces.py.  No tick of
any case raises one of the reference's crashing UBs (asserted with the oracle before every tick: pick another seed, do not filter).

  names str[G]  kind / horizon / simple_mask / first_mask int32[G]  result uint32[G, samples, 24]
  states uint8[2, 24, 1004]  moves int32[2, 24, 4]  dist int32[2]  seed int64  samples int32
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import rollout_policy_cases as PC  # noqa: E402
from tests import rollout_policy_oracle as PO  # noqa: E402
from tests.edge_states import FATAL  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "rollout_policy.npz")


def ref_lib():
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libpomref.so"))
    lib.ref_simple_new.restype = C.c_void_p
    lib.ref_simple_new.argtypes = [C.c_int, C.c_ulonglong]
    lib.ref_simple_delete.argtypes = [C.c_void_p]
    lib.ref_simple_peek_draw.argtypes = [C.c_void_p]
    lib.ref_simple_act.argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_simple_memory.argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_simple_set_memory.argtypes = [C.c_void_p, C.c_void_p]
    lib.ref_step.argtypes = [C.c_void_p, C.c_void_p]
    return lib


def main():
    ref = ref_lib()
    oracle = Oracle()
    name, mask, acts = [""], [0], [0]
    seed_for = {}   # (agent, draw) -> a generator seed whose first draw is that value

    def ref_step(s, mv):
        mv = np.ascontiguousarray(mv, dtype=np.int32)
        probe = s.copy()
        assert not oracle.step(probe, mv) & FATAL, name[0]
        ref.ref_step(s.ctypes.data, mv.ctypes.data)
        return 0

    def agent_with_draw(a, want):
        k = seed_for.get((a, want), 1)
        while True:
            obj = C.c_void_p(ref.ref_simple_new(a, k))
            if ref.ref_simple_peek_draw(obj) == want:
                seed_for[(a, want)] = k
                return obj
            ref.ref_simple_delete(obj)
            k += 1

    def ref_act(S, M, seed_r, env_offset, tick, done):
        out = np.zeros((S.size, 4), dtype=np.int32)
        for e in range(S.size):
            if done[e]:
                continue
            for a in range(4):
                if not mask[0] >> a & 1 or S["agents"]["dead"][e, a]:
                    continue
                obj = agent_with_draw(a, int(oracle.lib.pom_oracle_policy_draw(seed_r, env_offset + e, tick, a)))
                mem = np.ascontiguousarray(M[e, a])
                ref.ref_simple_set_memory(obj, mem.ctypes.data)
                out[e, a] = ref.ref_simple_act(obj, S[e:e + 1].ctypes.data)
                ref.ref_simple_memory(obj, mem.ctypes.data)
                M[e, a] = mem
                ref.ref_simple_delete(obj)
                acts[0] += 1
        return out

    oracle.lib.pom_oracle_policy_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    states = [PC.kind_states(oracle, i) for i in range(len(PC.KINDS))]
    moves = [PC.kind_moves(i) for i in range(len(PC.KINDS))]
    gs = PC.groups()
    result = np.zeros((len(gs), PC.SAMPLES, PC.PER_KIND), dtype=np.uint32)
    for g, grp in enumerate(gs):
        name[0], mask[0] = grp.name, grp.simple_mask
        result[g] = PO.rollout(oracle, states[grp.kind], None, grp.horizon, PC.SAMPLES, PC.SEED, PC.KINDS[grp.kind][2], grp.simple_mask,
                               grp.first_mask, moves[grp.kind] if grp.first_mask else None, step=ref_step, act=ref_act)
    # the fixture as a whole is not one-sided (another seed if it is; nothing is filtered)
    horizon = np.array([grp.horizon for grp in gs])
    a0_alive = np.stack([states[grp.kind]["agents"]["dead"][:, 0] == 0 for grp in gs])
    bal = PC.balance(result, horizon, a0_alive)
    assert PC.balanced(*bal), bal
    from tests import rollout_oracle as RO
    assert not (result & RO.RO_UB).any()
    np.savez_compressed(
        OUT,
        names=np.array([grp.name for grp in gs]), kind=np.array([grp.kind for grp in gs], dtype=np.int32),
        horizon=horizon.astype(np.int32), simple_mask=np.array([grp.simple_mask for grp in gs], dtype=np.int32),
        first_mask=np.array([grp.first_mask for grp in gs], dtype=np.int32), result=result,
        states=np.stack([np.frombuffer(s.tobytes(), dtype=np.uint8).reshape(PC.PER_KIND, 1004) for s in states]),
        moves=np.stack(moves).astype(np.int32), dist=np.array([k[2] for k in PC.KINDS], dtype=np.int32),
        seed=np.int64(PC.SEED), samples=np.int32(PC.SAMPLES),
    )
    print(f"rollout_policy.npz: {len(gs)} groups of {PC.SAMPLES} x {PC.PER_KIND} playouts, {acts[0]} reference act() calls; of "
          f"{bal[0]} words {bal[1]} finish early, {bal[2]} play all K ticks, {bal[3]} winners, {bal[4]} draws, agent 0 dies in {bal[5]}; "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
