"""TEST INFRASTRUCTURE — a host model of a handle under closed-loop range ticks (include/pom_batch.h pom_batch_step_device_range): per env
the state, the status (done, winner, draw, time-out, UB flags), the episode number, the terminal record with the last finished episode's
winner / draw / length / alive, and the `finished` mark; per handle the four counters (steps, episodes, resets, UB ticks).  tick() plays
one Environment::Step for the envs of a range ONLY, under the handle's options — POM_MODE_ENV, max_steps, auto_reset OFF / AT_START /
AT_END, fresh boards with their seed, env_offset — by the rules the header states; every other env keeps all it has.  Plain numpy plus
the CPU checker (Oracle.env_step, Oracle.boardgen).  Nothing of the kernels is restated: no tile, no column, no XCD.

The hooks (_snapshot_of, _board_env, _before_call, _count_restart) are there for the deliberately wrong variants of
tests/test_range_model_host.py, which show that the schedules of tests/range_cases.py tell a wrong kernel from a right one."""
import numpy as np

from pomcpp_amd.state import STATE_DTYPE
from tests import rollout_oracle as RO

RESET_OFF, RESET_AT_START, RESET_AT_END = 0, 1, 2
STATUS = ("done", "winner", "draw", "alive", "time_step", "ubflags")       # BatchEnvironment.status()
RESULTS = ("finished", "winner", "draw", "length", "alive")                 # BatchEnvironment.last_results()


def _clean(states):
    out = np.array(states, dtype=STATE_DTYPE)
    out["agents"]["pad"] = 0
    return out


class RangeModel:
    def __init__(self, oracle, start, *, max_steps=0, auto_reset=RESET_OFF, fresh_boards=False, board_seed=0, env_offset=0):
        """the handle after make_game(start) (or generate(): `start` are then the generated boards): the states are the restart
        snapshot, every status is clear, no episode has finished"""
        n = start.size
        self.oracle, self.n, self.max_steps, self.auto_reset = oracle, n, int(max_steps), auto_reset
        self.fresh, self.board_seed, self.env_offset = bool(fresh_boards), board_seed, env_offset
        self.states = _clean(start)
        self.snapshot = self.states.copy()
        self.done, self.winner, self.draw = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
        self.timeout, self.ubflags = np.zeros(n, np.int32), np.zeros(n, np.uint32)
        self.episodes = np.zeros(n, np.uint32)
        self.terminal = np.zeros(n, dtype=STATE_DTYPE)
        self.last = dict(winner=np.full(n, -1, np.int32), draw=np.zeros(n, np.int32), length=np.zeros(n, np.int32), alive=np.zeros(n, np.int32))
        self.finished = np.zeros(n, np.int32)
        self.counters = np.zeros(4, np.int64)   # steps, episodes, resets, UB ticks
        self.calls = []                         # what every tick() did: the schedule conditions are read off this

    # ---- the places where a kernel addresses by env (the wrong variants override them) ----------------------------------------
    def _snapshot_of(self, e, first):
        return self.snapshot[e]

    def _board_env(self, e, first):
        """the env's number in the whole job: what keys its boards"""
        return self.env_offset + e

    def _before_call(self, first, count):
        pass

    def _count_restart(self, e):
        self.counters[2] += 1

    # ---- one call ----------------------------------------------------------------------------------------------------------------
    def _restart(self, e, first, log):
        if self.fresh:
            self.episodes[e] += 1
            self.states[e] = self.oracle.boardgen(self.board_seed, [self._board_env(e, first)], [int(self.episodes[e])])[0]
        else:
            self.states[e] = self._snapshot_of(e, first)
        self.done[e], self.winner[e], self.draw[e], self.timeout[e], self.ubflags[e] = 0, -1, 0, 0, 0   # a restart starts an episode
        self._count_restart(e)
        log["restarted"].append(e)

    def tick(self, first, count, moves):
        """one pom_batch_step_device_range(first, count, moves): `moves` int32 [n, 4], indexed by the env's number in the batch"""
        assert 0 <= first and count >= 0 and first + count <= self.n
        moves = np.asarray(moves, dtype=np.int32)
        assert moves.shape == (self.n, 4)
        outside = np.ones(self.n, bool)
        outside[first:first + count] = False
        log = dict(first=first, count=count, restarted=[], ticked=0, by_deaths=0, marked_outside=int((self.finished[outside] != 0).sum()))
        self._before_call(first, count)
        for e in range(first, first + count):
            if self.done[e]:
                if self.auto_reset != RESET_AT_START:
                    continue                     # OFF: a finished env is skipped and not counted (AT_END leaves nobody finished)
                self._restart(e, first, log)     # AT_START: it restarts before its next own tick
            self.finished[e] = 0                 # the env's own tick clears its mark, and nothing else does
            st = dict(done=0, winner=-1, draw=0)
            ub = self.oracle.env_step(self.states[e:e + 1], moves[e], st)
            self.states["agents"]["pad"][e] = 0
            self.counters[0] += 1
            self.counters[3] += ub != 0
            self.ubflags[e] |= ub
            self.timeout[e] = self.max_steps > 0 and int(self.states["timeStep"][e]) >= self.max_steps
            self.done[e], self.winner[e], self.draw[e] = st["done"] or self.timeout[e], st["winner"], st["draw"]
            log["ticked"] += 1
            if self.done[e]:
                self.counters[1] += 1
                log["by_deaths"] += st["done"]
                if self.auto_reset == RESET_AT_END:   # the tick that finishes an episode keeps its end, restarts the env and marks it
                    self.terminal[e] = self.states[e]
                    self.last["winner"][e], self.last["draw"][e] = self.winner[e], self.draw[e]
                    self.last["length"][e], self.last["alive"][e] = self.states["timeStep"][e], self.states["aliveAgents"][e]
                    self._restart(e, first, log)
                    self.finished[e] = 1
        self.calls.append(log)
        return log

    def random_ticks(self, seed, dist, tick0, ticks):
        """pom_batch_step_random(seed, dist, ticks) of a handle whose tick is tick0: whole-batch ticks with the pom_rng.h stream"""
        for t in range(ticks):
            self.tick(0, self.n, [RO.rng_moves(seed, self.env_offset + e, tick0 + t, dist) for e in range(self.n)])

    # ---- everything the API can read --------------------------------------------------------------------------------------------
    def readable(self):
        out = dict(state=self.states, episodes=self.episodes, counters=self.counters)
        out.update(status_done=self.done, status_winner=self.winner, status_draw=self.draw, status_alive=self.states["aliveAgents"].astype(np.int32),
                   status_time_step=self.states["timeStep"].astype(np.int32), status_ubflags=self.ubflags)
        if self.auto_reset == RESET_AT_END:
            out.update(terminal=self.terminal, last_finished=self.finished, **{"last_" + k: v for k, v in self.last.items()})
        return out

    def read_handle(self, env):
        """readable() of a BatchEnvironment (the calls synchronise the handle)"""
        out = dict(state=env.get_state(), episodes=env.episodes(), counters=env.counters())
        out.update({"status_" + k: v for k, v in env.status().items()})
        if self.auto_reset == RESET_AT_END:
            out.update(terminal=env.get_terminal_state(), **{"last_" + k: v for k, v in env.last_results().items()})
        return out

    def differences(self, other):
        """the names of what differs between this model and `other` (a model, or read_handle()'s dict)"""
        mine, theirs = self.readable(), other.readable() if isinstance(other, RangeModel) else other
        assert set(mine) == set(theirs) and set(mine) >= {"state", "episodes", "counters"} | {"status_" + k for k in STATUS}
        return [k for k in mine if np.asarray(mine[k]).tobytes() != np.asarray(theirs[k]).astype(np.asarray(mine[k]).dtype).tobytes()]

    def same_as(self, env, what=""):
        """everything the API can read of the handle is the model's: get_state, status (all six arrays), episodes, counters (all four)
        and, with AT_END, last_results (all five arrays) and get_terminal_state"""
        got, mine = self.read_handle(env), self.readable()
        bad = self.differences(got)
        if bad:
            k = bad[0]
            g, w = np.asarray(got[k]), np.asarray(mine[k])
            where = np.nonzero(g.view(np.uint8).reshape(g.shape[0], -1) != w.astype(g.dtype).view(np.uint8).reshape(g.shape[0], -1))[0]
            detail = f"counters {g.tolist()} != {w.tolist()}" if k == "counters" else f"first at index {int(where[0])} of {np.unique(where).size} that differ"
            if k in ("state", "terminal"):
                e = int(where[0])
                detail += f", fields {[f for f in g.dtype.names if g[e][f].tobytes() != w[e][f].tobytes()]}"
            raise AssertionError(f"{what}: {bad} differ; {k}: {detail}")
