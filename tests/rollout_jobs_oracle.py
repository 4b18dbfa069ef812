"""TEST INFRASTRUCTURE — the checker of pom_batch_rollout_jobs (include/pom_batch.h PomRolloutJobsSpec), by the header's reduction:
job j is tests/rollout_policy_oracle.rollout on the ONE state src[j] with the job's own moves of tick 1, its draws keyed by
env_offset + src[j]; an entry outside 0 .. n - 1 is "no job" and gives zeros.  Nothing of the kernel is restated: no tile, no gather,
no group of 16."""
import numpy as np

from tests import rollout_policy_oracle as PO

RO_NONE = 0


def golden_jobs(n, m=37, seed=5):
    """m sources out of n with repeats, in no order (the host's and the GPU's test of the fixture share it)"""
    src = np.random.default_rng(seed).integers(0, n, m).astype(np.int64)
    src[[3, 11, 30]] = src[0]        # one source several times, within a group of 16 and beyond it
    return src


def rollout_jobs(oracle, states, mems, src, horizon, samples, seed, dist, simple_mask, first_mask=0, moves=None, max_steps=0,
                 env_offset=0, start=None):
    """states STATE_DTYPE[n], mems int32[n, 4, 16] or None (fresh agents), src int[m], moves int32[m, 4] PER JOB or None; start: uint32[n]
    or None, the status of the envs' S_0 as in rollout_policy_oracle.rollout -> uint32[samples, m]"""
    n, src = states.size, np.asarray(src, dtype=np.int64)
    out = np.full((samples, src.size), RO_NONE, dtype=np.uint32)
    for j, s in enumerate(src.tolist()):
        if not 0 <= s < n:
            continue
        out[:, j] = PO.rollout(oracle, states[s:s + 1], None if mems is None else mems[s:s + 1], horizon, samples, seed, dist, simple_mask,
                               first_mask, None if moves is None else moves[j:j + 1], max_steps, env_offset + s,
                               None if start is None else start[s:s + 1])[:, 0]
    return out
