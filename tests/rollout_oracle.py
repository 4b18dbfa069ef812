"""TEST INFRASTRUCTURE — the checker of pom_batch_rollout (include/pom_batch.h PomRolloutSpec): for every env and sample, up to
K x Oracle.step on a copy of the state under the pom_rng.h move stream (restated here in a dozen lines), with Environment::Step's
bookkeeping after every tick, packed into the result word.  The tick is the oracle's; nothing of the kernel is restated."""
import numpy as np

M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
DIST_HARMLESS, DIST_RANDOM, DIST_STRESS = 0, 1, 2
# the result word (POM_RO_* of the header)
RO_DONE, RO_DRAW, RO_TIMEOUT, RO_UB, RO_WINNER_SHIFT, RO_LENGTH_SHIFT = 0x10, 0x20, 0x40, 0x80, 8, 16


# ---- include/pom_rng.h ----
def splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def fmix32(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def draw_half(seed, env, tick, upper):
    k = (seed & M32) ^ ((env * 0x9E3779B1) & M32) ^ ((tick * 0x7FEB352D + (seed >> 32)) & M32)
    return fmix32(k ^ 0x68E31DA4 if upper else k)


def pick(r16, dist):
    if dist == DIST_STRESS:
        return sum(r16 >= edge for edge in (6554, 16384, 26214, 36045, 45875))
    return (r16 * (5 if dist == DIST_HARMLESS else 6)) >> 16


def rng_moves(seed, env, tick, dist):
    """pom_rng_moves: Move[4] of (seed, env, tick)"""
    lo, hi = draw_half(seed, env & M32, tick, 0), draw_half(seed, env & M32, tick, 1)
    return [pick(lo & 0xFFFF, dist), pick(lo >> 16, dist), pick(hi & 0xFFFF, dist), pick(hi >> 16, dist)]


def alive_bits(state):
    return sum((not int(d)) << a for a, d in enumerate(state["agents"][0]["dead"]))


def rollout(oracle, states, horizon, samples, seed, dist, moves=None, max_steps=0, env_offset=0, start=None, step=None):
    """states STATE_DTYPE[n] (not changed); moves int32[n, 4] of tick 1 of every sample, or None; start: uint32[n] or None, the status
    of S_0 in the result word's bits (an env with RO_DONE there is finished at S_0: length 0, these bits and its alive agents in every
    sample) -> the result words uint32[samples, n].  `step(state, moves) -> flags` replaces the oracle's step (the fixture's generator
    plays the compiled reference)."""
    n = states.size
    step = step or oracle.step
    out = np.zeros((samples, n), dtype=np.uint32)
    for r in range(samples):
        seed_r = splitmix64((seed + r) & M64)
        for e in range(n):
            s = states[e:e + 1].copy()
            word = int(start[e]) if start is not None else 0
            length = ub = 0
            for t in range(1, horizon + 1):
                if word & RO_DONE:   # Environment::Step returns early, environment.cpp:125-128
                    break
                mv = moves[e] if t == 1 and moves is not None else rng_moves(seed_r, env_offset + e, t - 1, dist)
                ub |= int(step(s, np.asarray(mv, dtype=np.int32)))
                s["timeStep"] += 1   # environment.cpp:150
                length = t
                alive = int(s["aliveAgents"][0])
                if alive == 1:       # :152-163: the last alive index wins
                    word |= RO_DONE | (max(a for a in range(4) if not s["agents"][0, a]["dead"]) + 1) << RO_WINNER_SHIFT
                if alive == 0:       # :164-168
                    word |= RO_DONE | RO_DRAW
                if max_steps > 0 and int(s["timeStep"][0]) >= max_steps:   # StartGame's bound, environment.cpp:71
                    word |= RO_DONE | RO_TIMEOUT
            out[r, e] = word | alive_bits(s) | (RO_UB if ub else 0) | length << RO_LENGTH_SHIFT
    return out
