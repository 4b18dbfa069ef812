"""TEST INFRASTRUCTURE — what the GPU tests of the two rollout entry points (tests/test_rollout.py, tests/test_rollout_policy.py)
share: the played boards, a handle holding them, tensors to and from the device, the word-by-word comparison and the dump of all
the API can read of a handle."""
import functools

import numpy as np

from tests import forecast_cases as FC

POOL = 200                        # the batches of every size are the first n states of one pool: env e has the same key in all


@functools.lru_cache(maxsize=None)
def _played(kind, ticks, n=POOL):
    from tests.oracle_lib import Oracle
    s = FC.played_states(Oracle(), kind, n, ticks)
    s.setflags(write=False)
    return s


def _env(states, **kw):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    kw.setdefault("mode", MODE_ENV)
    env = BatchEnvironment(len(states), **kw)
    env.make_game(states)
    return env


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, what):
    got = _words(got)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} words differ, first (sample, env) {bad[0].tolist()}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}"


def _everything(env):
    """all the API can read of a handle"""
    out = dict(state=env.get_state().tobytes(), terminal=env.get_terminal_state().tobytes(), counters=env.counters().tolist(),
               episodes=env.episodes().tolist(), memory=env.policy_memory().tobytes(), chain=env.chain_stats())
    out.update({"status_" + k: v.tolist() for k, v in env.status().items()})
    out.update({"last_" + k: v.tolist() for k, v in env.last_results().items()})
    return out
