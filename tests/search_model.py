"""TEST INFRASTRUCTURE — a host model of a handle under the search calls (include/pom_batch.h PomExpandSpec, PomRolloutJobsSpec): the
states, the statuses, the SimpleAgent memory, the episode counters, the terminal records and the first three counters of a batch, and
what expand, an explicit-move tick and rollout_jobs make of them.  Plain numpy plus the CPU checker: the tick is tests/expand_oracle.py's,
the playouts are tests/rollout_jobs_oracle.py's; what is restated here is the header's copy rule of the side arrays — a job that copies
(src != destination) gives its destination the source's memory, episode counter and terminal record, read BEFORE the call — and the
masked-step equivalence: a tick of the whole batch without restarts is expand with the identity list.  Nothing of the kernels is
restated: no tile, no gather, no column."""
import numpy as np

from pomcpp_amd.state import STATE_DTYPE
from tests import expand_oracle as XO
from tests import rollout_jobs_oracle as JO
from tests import rollout_oracle as RO


def status_of(handle_status, max_steps=0):
    """XO.blank_status' arrays from what BatchEnvironment.status() returns: the API reports no time-out, a finished game whose
    timeStep has reached the bound has one (environment.cpp:71)"""
    n = len(handle_status["done"])
    st = XO.blank_status(n)
    for k in ("done", "winner", "draw"):
        st[k][:] = handle_status[k]
    st["ubflags"][:] = handle_status["ubflags"]
    if max_steps > 0:
        st["timeout"][:] = (handle_status["done"] != 0) & (handle_status["time_step"] >= max_steps)
    return st


def start_words(status):
    """the statuses in the result word's bits: rollout_policy_oracle.rollout's `start`"""
    return ((status["done"] != 0) * RO.RO_DONE | (status["draw"] != 0) * RO.RO_DRAW | (status["timeout"] != 0) * RO.RO_TIMEOUT |
            (status["winner"].astype(np.int64) + 1) << RO.RO_WINNER_SHIFT).astype(np.uint32)


def terminal_of(env):
    """the terminal records, or None: only a POM_RESET_AT_END handle keeps them"""
    from pomcpp_amd.batch import PomError
    try:
        return env.get_terminal_state()
    except PomError:
        return None


def everything(env):
    """tests/rollout_gpu._everything for a handle of any reset mode: all the API can read of it"""
    t = terminal_of(env)
    out = dict(state=env.get_state().tobytes(), terminal=None if t is None else t.tobytes(), counters=env.counters().tolist(),
               episodes=env.episodes().tolist(), memory=env.policy_memory().tobytes(), chain=env.chain_stats())
    out.update({"status_" + k: v.tolist() for k, v in env.status().items()})
    if t is not None:
        out.update({"last_" + k: v.tolist() for k, v in env.last_results().items()})
    return out


class SearchModel:
    def __init__(self, oracle, states, mode=XO.MODE_ENV, max_steps=0, status=None, memory=None, episodes=None, terminal=None):
        n = states.size
        self.oracle, self.mode, self.max_steps, self.n = oracle, mode, max_steps, n
        self.states = np.array(states, dtype=STATE_DTYPE)
        self.status = XO.blank_status(n) if status is None else {k: np.array(v) for k, v in status.items()}
        self.memory = np.zeros((n, 4, 16), dtype=np.int32) if memory is None else np.array(memory, dtype=np.int32)
        self.episodes = np.zeros(n, dtype=np.uint32) if episodes is None else np.array(episodes, dtype=np.uint32)
        self.terminal = np.zeros(n, dtype=STATE_DTYPE) if terminal is None else np.array(terminal, dtype=STATE_DTYPE)
        self.counters = [0, 0, 0]               # steps, episodes, resets

    @classmethod
    def of_handle(cls, oracle, env, mode, max_steps):
        """the model of a handle as it stands (the handle is synchronised)"""
        m = cls(oracle, env.get_state(), mode, max_steps, status_of(env.status(), max_steps), env.policy_memory(), env.episodes(),
                terminal_of(env))
        m.counters = env.counters().tolist()[:3]
        return m

    def expand(self, src, moves, first):
        """-> the result words uint32 [count]"""
        src = np.asarray(src, dtype=np.int64)
        count = src.size
        before = self.memory.copy(), self.episodes.copy(), self.terminal.copy()
        self.states, self.status, words, ticks, newly = XO.expand(self.oracle, self.states, self.status, src, moves, first, self.mode,
                                                                  self.max_steps)
        for j in range(count):
            s, d = int(src[j]), first + j
            if XO.is_job(s, d, first, count, self.n) and s != d:
                self.memory[d], self.episodes[d], self.terminal[d] = before[0][s], before[1][s], before[2][s]
        self.counters[0] += ticks
        self.counters[1] += newly
        return words

    def step(self, moves):
        """one explicit-move tick of the whole batch, no restart: the masked step over every env -> the result words uint32 [n]"""
        return self.expand(np.arange(self.n, dtype=np.int64), moves, 0)

    def rollout_jobs(self, src, horizon, samples, seed, dist=RO.DIST_RANDOM, simple=0, first=0, moves=None, env_offset=0):
        """-> uint32 [samples, m]; the model is not changed"""
        return JO.rollout_jobs(self.oracle, self.states, self.memory, src, horizon, samples, seed, dist, simple, first, moves,
                               self.max_steps, env_offset, start_words(self.status))

    def same_as(self, env, what=""):
        """everything the API can read of the handle is the model's (the counters: the first three)"""
        got, st = env.get_state(), env.status()
        assert got.tobytes() == self.states.tobytes(), (what, "state", np.nonzero(got.view(np.uint8).reshape(self.n, -1) !=
                                                                                   self.states.view(np.uint8).reshape(self.n, -1))[0][:8])
        for k in ("done", "winner", "draw", "ubflags"):
            assert np.array_equal(st[k], self.status[k]), (what, k)
        assert np.array_equal(st["alive"], self.states["aliveAgents"]) and np.array_equal(st["time_step"], self.states["timeStep"]), what
        assert env.policy_memory().tobytes() == self.memory.tobytes(), (what, "memory")
        assert np.array_equal(env.episodes(), self.episodes), (what, "episodes")
        t = terminal_of(env)
        assert t is None or t.tobytes() == self.terminal.tobytes(), (what, "terminal")
        assert env.counters().tolist()[:3] == self.counters, (what, "counters", env.counters().tolist(), self.counters)
