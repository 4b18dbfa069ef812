"""Inputs of the policy-rollout tests (pom_batch_rollout_policy, include/pom_batch.h PomRolloutPolicySpec) — test infrastructure,
numpy only.

groups(): the fixture's entries — the boards of tests/rollout_cases.KINDS (24 per kind), rolled out at three horizons under three
configurations: all four agents SimpleAgent; agent 0 on the kind's random stream; the same with agent 0's first move given.
tests/golden/gen_rollout_policy.py plays them with the compiled reference's Step and SimpleAgent."""
from __future__ import annotations

from dataclasses import dataclass

from tests import rollout_cases as RC

SEED, SAMPLES, PER_KIND = 99, 4, RC.PER_KIND
HORIZONS = RC.HORIZONS
KINDS = RC.KINDS
# (name, simple_mask, first_mask)
CONFIGS = (("all", 0xF, 0x0), ("a0rnd", 0xE, 0x0), ("a0first", 0xE, 0x1))


@dataclass
class Group:
    name: str
    kind: int          # index into KINDS
    horizon: int
    simple_mask: int
    first_mask: int


def groups():
    return [Group(f"{kind}{ticks}_K{k}_{cname}", i, k, sm, fm)
            for i, (kind, ticks, _) in enumerate(KINDS) for k in HORIZONS for cname, sm, fm in CONFIGS]


def kind_states(oracle, i, n=PER_KIND):
    return RC.kind_states(oracle, i, n)


def kind_moves(i, n=PER_KIND):
    return RC.kind_moves(i, n)


def balance(result, horizon, a0_alive):
    """what the fixture as a whole must hold (result uint32[G, R, n], horizon int[G], a0_alive bool[G, n]: agent 0 alive in S_0):
    -> (size, words that finish before K, words that play all K ticks, winners, draws, words in which agent 0 dies during the playout)"""
    from tests import rollout_oracle as RO
    length, k = result >> RO.RO_LENGTH_SHIFT, horizon[:, None, None]
    early, full = int(((result & RO.RO_DONE != 0) & (length < k)).sum()), int((length == k).sum())
    winners, draws = int((result >> RO.RO_WINNER_SHIFT & 7 != 0).sum()), int((result & RO.RO_DRAW != 0).sum())
    a0_dies = int((a0_alive[:, None, :] & (result & 1 == 0)).sum())
    return result.size, early, full, winners, draws, a0_dies


def balanced(size, early, full, winners, draws, a0_dies):
    return 8 * early >= size and 8 * full >= size and winners >= 10 and draws >= 1 and a0_dies >= 10
