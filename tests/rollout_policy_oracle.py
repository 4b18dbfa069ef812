"""TEST INFRASTRUCTURE — the checker of pom_batch_rollout_policy (include/pom_batch.h PomRolloutPolicySpec): tests/rollout_oracle.rollout
plus the three move sources.  For every sample, up to K times: Oracle.simple_policy asks the live agents of the envs still playing
(the oracle's restatement of SimpleAgent, its draw from the pom_rng.h stream, its memory carried in `mems`), the agents outside
simple_mask get RO.rng_moves' entry, the agents of first_mask get the caller's move on tick 1; then Oracle.step and Environment::Step's
bookkeeping, packed into rollout_oracle's result word.  The tick and the policy are the oracle's; nothing of the kernel is restated."""
import numpy as np

from tests import rollout_oracle as RO


def mask_of(agents):
    return sum(1 << a for a in agents)


def fresh_memory(n):
    return np.zeros((n, 4, 16), dtype=np.int32)


def rollout(oracle, states, mems, horizon, samples, seed, dist, simple_mask, first_mask=0, moves=None, max_steps=0, env_offset=0,
            start=None, step=None, act=None):
    """states STATE_DTYPE[n] and mems int32[n, 4, 16] (neither is changed; mems None = fresh agents); moves int32[n, 4], read on tick 1
    for the agents of first_mask; start: uint32[n] or None, the status of S_0 in the result word's bits, as in rollout_oracle.rollout
    -> the result words uint32[samples, n].  `step(state, moves) -> flags` and `act(states, mems, seed_r, env_offset, tick, done) ->
    int32[n, 4]` replace the oracle's (the fixture's generator plays the compiled reference)."""
    n = states.size
    step = step or oracle.step
    act = act or oracle.simple_policy
    assert 0 <= simple_mask <= 15 and 0 <= first_mask <= 15 and (first_mask == 0 or moves is not None)
    out = np.zeros((samples, n), dtype=np.uint32)
    for r in range(samples):
        seed_r = RO.splitmix64((seed + r) & RO.M64)
        S = states.copy()
        M = fresh_memory(n) if mems is None else np.ascontiguousarray(mems, dtype=np.int32).copy()
        word = np.zeros(n, dtype=np.int64) if start is None else np.asarray(start).astype(np.int64)
        length, ub = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
        for t in range(1, horizon + 1):
            done = (word & RO.RO_DONE) != 0          # Environment::Step returns early, environment.cpp:125-128
            if done.all():
                break
            # live agents of the envs still playing are asked; a dead agent's entry is IDLE (environment.cpp:139-146)
            asked = act(S, M, seed_r, env_offset, t - 1, done.astype(np.int32)) if simple_mask else None
            for e in np.nonzero(~done)[0]:
                stream = RO.rng_moves(seed_r, env_offset + int(e), t - 1, dist)
                mv = [int(asked[e, a]) if simple_mask >> a & 1 else stream[a] for a in range(4)]
                if t == 1:
                    mv = [int(moves[e][a]) if first_mask >> a & 1 else mv[a] for a in range(4)]
                s = S[e:e + 1]
                ub[e] |= bool(step(s, np.asarray(mv, dtype=np.int32)))
                s["timeStep"] += 1                   # environment.cpp:150
                length[e] = t
                alive = int(s["aliveAgents"][0])
                if alive == 1:                       # :152-163: the last alive index wins
                    word[e] |= RO.RO_DONE | (max(a for a in range(4) if not s["agents"][0, a]["dead"]) + 1) << RO.RO_WINNER_SHIFT
                if alive == 0:                       # :164-168
                    word[e] |= RO.RO_DONE | RO.RO_DRAW
                if max_steps > 0 and int(s["timeStep"][0]) >= max_steps:   # StartGame's bound, environment.cpp:71
                    word[e] |= RO.RO_DONE | RO.RO_TIMEOUT
        for e in range(n):
            out[r, e] = int(word[e]) | RO.alive_bits(S[e:e + 1]) | (RO.RO_UB if ub[e] else 0) | int(length[e]) << RO.RO_LENGTH_SHIFT
    return out
