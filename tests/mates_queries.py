"""TEST INFRASTRUCTURE — the chosen wavefront-mates of tests/tile_mates.py as inputs of every kernel that embeds the tick in an LDS array of
its own: pom_step_mixed_kernel, pom_rollout_policy_kernel (both forms and JOBS), pom_rollout_kernel, pom_move_safety_kernel,
pom_forecast_kernel, pom_expand_kernel and the fogged export of the step kernels (tests/test_gpu_mates_queries.py).  Numpy only, no GPU.

The batch is the one tests/test_tile_mates._whole(cast, 16) builds: the EPW-16 families overlay (1,440 envs), pairs (1,536), restart
(160) and crowd with tail 5 (245) — 3,381 envs, 110 of the 112 actors, the last tile short.  "The batch at tick t0" holds, for t0 = 0,
every env's actor's start state and, for t0 = 1, the actor's solo trace after its first tick; the first tick played on either is the
actor's decisive one (the deep_b / select / claims_full actors go off on tick 0, their push1 / select1 / top1 variants on tick 1), and
"the moves" are row t0 of the actor's script.  at(t0) is an edge_queries.Queries with order = the composition, so every per-state
checker of tests/edge_queries.py is reused and gathered by the composition; what is keyed by the env (the rollouts) runs on the placed
batch.  Everything is computed once, kept, and never written again."""
import numpy as np

from pomcpp_amd.state import STATE_DTYPE
from tests import edge_queries as EQ
from tests import expand_oracle as XO
from tests import rollout_jobs_oracle as JO
from tests import rollout_oracle as RO
from tests import rollout_policy_oracle as PO
from tests import tile_mates as TM
from tests import view_oracle as VO
from tests.mixed_model import MixedModel

SEED = EQ.SEED
T0S = (0, 1)
MASKS = (0b0110, 0xF)                      # the SimpleAgent masks of the mixed step
VIEW_RADIUS = 4
ROLLOUT_K, ROLLOUT_R = EQ.ROLLOUT_K, EQ.ROLLOUT_R      # 24 ticks, 2 samples, DIST_STRESS after the moves
POLICY_K, POLICY_R, POLICY_MASK = 12, 1, 0b1010       # SimpleAgents in seats 1 and 3
JOBS_SIMPLE, JOBS_FIRST = 0b0100, 0xF
SAFETY_K = EQ.SAFETY_K
BOARD_SEED = 31                            # the fresh boards of the restart family


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


class Mates:
    """stage: tests/test_tile_mates.Stage (actors, cast, solo traces, sticky flags); fam / who: family name and actor of every env"""

    def __init__(self, oracle):
        from tests.test_tile_mates import Stage, _whole   # (the batch IS that module's: built by its own function)
        self.oracle, self.stage = oracle, Stage(oracle)
        self.fam, self.who = _whole(self.stage.cast, 16)
        self.who = _frozen(self.who.astype(np.int64))
        self.n, self.actors = self.who.size, len(self.stage.entries)
        self.names = self.stage.cast.names
        self.start, self.script = _frozen(*TM.batch(self.stage.entries, self.who))   # STATE_DTYPE [n], int32 [T, n, 4]
        self._kept = {}

    def _once(self, key, make):
        if key not in self._kept:
            v = make()
            _frozen(*(v if isinstance(v, tuple) else (v,)))
            self._kept[key] = v
        return self._kept[key]

    # ---- the inputs ------------------------------------------------------------------------------------------------------------------
    def distinct(self, t0):
        """the 112 actors' states at tick t0 and the moves each plays next: STATE_DTYPE [A], int32 [A, 4]"""
        def make():
            if t0 == 0:
                states = np.concatenate([e.start for e in self.stage.entries])
            else:
                states = np.ascontiguousarray(self.stage.states[:, t0 - 1]).view(STATE_DTYPE).reshape(-1)
            return states.copy(), np.stack([e.moves[t0] for e in self.stage.entries]).astype(np.int32)
        return self._once(("distinct", t0), make)

    def at(self, t0):
        """the batch at tick t0 as Queries: placed = the 3,381 envs, order = the composition"""
        def make():
            states, moves = self.distinct(t0)
            return EQ.Queries(self.oracle, [f"{n}@{t0}" for n in self.names], states, moves, order=self.who)
        return self._once(("at", t0), make)

    def once_each(self, t0):
        """the 112 states once each, in the actors' order (7 whole tiles): the handle of the jobs' and expand's tests"""
        def make():
            states, moves = self.distinct(t0)
            return EQ.Queries(self.oracle, [f"{n}@{t0}" for n in self.names], states, moves, order=np.arange(self.actors))
        return self._once(("once", t0), make)

    def name_of_env(self, k):
        k = int(k)
        mates = [self.names[i] for i in self.who[k - k % 16:k - k % 16 + 16]]
        return f"{self.fam[k]}: env {k} (wavefront {k // 16}, column {k % 16}) actor {self.names[self.who[k]]}; its wavefront: {mates}"

    # ---- the mixed step ------------------------------------------------------------------------------------------------------------------
    def model(self, **options):
        """a fresh host model of a MODE_ENV handle after make_game(the batch at tick 0)"""
        return MixedModel(self.oracle, self.start, **options)

    def played(self, mask, ticks=TM.TICKS):
        """MixedModel (MODE_ENV, no reset, cap 0), the scripts for the agents outside `mask`, tick t of the call = t: per tick the states
        uint8 [ticks, n, 1004], the sticky flags, done and the agents' memory"""
        def make():
            fr = [f.readable() for f in self.frames(mask, ticks)]
            return (np.stack([f["state"].view(np.uint8).reshape(self.n, 1004) for f in fr]), np.stack([f["status_ubflags"] for f in fr]),
                    np.stack([f["status_done"] for f in fr]), np.stack([f["memory"] for f in fr]))
        return self._once(("played", mask, ticks), make)

    def views(self, states):
        """the fused fogged codes (radius 4) of downloaded or model states: codes uint8 [n, 4, 5, 11, 11], viewer_attrs int32 [n, 4, 12],
        env_attrs' timeStep and aliveAgents int32 [n, 2] — view_oracle on the observe oracle's unfogged outputs"""
        ob = EQ.observe_oracle()
        states = np.ascontiguousarray(states).view(STATE_DTYPE).reshape(-1)
        _, attrs, env2 = ob.observe(states)
        return VO.view_codes(ob.observe_codes(states), attrs, VIEW_RADIUS), VO.viewer_attrs(attrs, env2[:, 0]), env2

    def planes_f16(self, states):
        """the per-agent float16 planes of downloaded or model states: planes [n, 4, 16, 11, 11], agent_attrs, env_attrs' first two"""
        states = np.ascontiguousarray(states).view(STATE_DTYPE).reshape(-1)
        return EQ.observe_oracle().observe(states, per_agent=True, dtype=np.float16)

    def trace_views(self, t):
        """views() of the 112 solo traces after tick t (gather with `who`: an env's state under its script is its actor's trace)"""
        return self._once(("trace_views", t), lambda: self.views(self.stage.states[:, t]))

    def trace_planes(self, t):
        return self._once(("trace_planes", t), lambda: self.planes_f16(self.stage.states[:, t]))

    def restarts(self, mode, mask, ticks=3 * TM.ENV_CAP + 2):
        """the restart family (the envs of fam == "restart", whole tiles) under a cap of ENV_CAP; mode: (auto_reset, fresh_boards);
        -> per whole-range mixed tick (everything the API can read after it, the envs it restarted)"""
        def make():
            lo, cnt = self.family("restart")
            auto_reset, fresh = mode
            m = MixedModel(self.oracle, self.start[lo:lo + cnt], max_steps=TM.ENV_CAP, auto_reset=auto_reset, fresh_boards=fresh,
                           board_seed=BOARD_SEED)
            frames = []
            for t in range(ticks):
                log = m.tick_mixed(0, cnt, self.restart_moves(t), mask, SEED, t)
                frames.append((Frozen(m), tuple(log["restarted"])))
            return tuple(frames)
        return self._once(("restarts", mode, mask, ticks), make)

    def frames(self, mask, ticks=TM.TICKS):
        """the whole batch on a MODE_ENV handle without reset under whole-batch mixed ticks (the scripts for the agents outside `mask`,
        call t at tick t): everything the API can read after every call"""
        def make():
            m, out = self.model(), []
            for t in range(ticks):
                m.tick_mixed(0, self.n, self.script[t], mask, SEED, t)
                out.append(Frozen(m))
            return tuple(out)
        return self._once(("frames", mask, ticks), make)

    def family(self, name):
        """(first env, count) of a family: each is one run of whole tiles (the ragged crowd last)"""
        idx = np.nonzero(np.array(self.fam) == name)[0]
        assert idx.size and np.array_equal(idx, np.arange(idx[0], idx[0] + idx.size)) and idx[0] % 16 == 0
        return int(idx[0]), int(idx.size)

    def restart_moves(self, t):
        """the restart family's moves of call t: the scripts, IDLE once a script has ended (every actor of the family idles throughout)"""
        lo, cnt = self.family("restart")
        return self.script[t, lo:lo + cnt] if t < self.script.shape[0] else np.zeros((cnt, 4), np.int32)

    # ---- the search calls on the batch -----------------------------------------------------------------------------------------------------
    def memory(self, t0):
        """the agents' memory after policy_simple(SEED) on a fresh handle at tick t0's batch (handle tick 0) — what one step_simple tick
        leaves on a twin, no env restarting: int32 [n, 4, 16], and the policy's moves"""
        def make():
            mems = np.zeros((self.n, 4, 16), np.int32)
            moves = self.oracle.simple_policy(self.at(t0).placed.copy(), mems, SEED, 0, 0)
            return mems, np.asarray(moves, dtype=np.int32)
        return self._once(("memory", t0), make)

    def rollout_policy(self, t0, fresh):
        def make():
            q = self.at(t0)
            return PO.rollout(self.oracle, q.placed, None if fresh else self.memory(t0)[0], POLICY_K, POLICY_R, SEED, RO.DIST_RANDOM, POLICY_MASK)
        return self._once(("rollout_policy", t0, fresh), make)

    # ---- the company made by the gather / by the jobs ------------------------------------------------------------------------------------
    def jobs(self, t0):
        """on the handle of once_each(t0): the source list IS the composition (3,381 jobs: job group g is wavefront g of the batch, put
        together column by column), 11 entries that are no job, and the 112 envs in order (7 groups that are a tile in order: loaded,
        not gathered).  Every job plays its state's next moves; fresh agents.  By the header's reduction a job's words depend on its
        source and its moves alone, so the checker is asked once per distinct (source, moves) and the answers are gathered.
        -> (src int64 [m], moves int32 [m, 4], words uint32 [ROLLOUT_R, m])"""
        def make():
            h = self.once_each(t0)
            src = np.concatenate([self.who, np.full(11, -1, np.int64), np.arange(self.actors, dtype=np.int64)])
            assert (self.n + 11) % 16 == 0
            ok = src >= 0
            mv = np.zeros((src.size, 4), np.int32)
            mv[ok] = h.moves[src[ok]]
            per_state = JO.rollout_jobs(self.oracle, h.states, None, np.arange(self.actors), ROLLOUT_K, ROLLOUT_R, SEED, RO.DIST_STRESS,
                                        JOBS_SIMPLE, JOBS_FIRST, h.moves)
            words = np.full((ROLLOUT_R, src.size), JO.RO_NONE, np.uint32)
            words[:, ok] = per_state[:, src[ok]]
            return src, mv, words
        return self._once(("jobs", t0), make)

    def expand(self, mode):
        """the handle holds the 112 start states and 3,381 slots behind them.  Call 0: slot j becomes the child of env who[j] under
        script row 0 (the job columns are the composition's).  Call 1: the identity list, the masked step of every slot, script row 1.
        -> [(src, moves, batch after the call, statuses, words)] of the two calls, by expand_oracle"""
        def make():
            h = self.once_each(0)
            both = np.concatenate([h.states, np.zeros(self.n, dtype=STATE_DTYPE)])
            out, status = [], None
            for src, mv in ((self.who, self.script[0]), (np.arange(self.actors, self.actors + self.n, dtype=np.int64), self.script[1])):
                both, status, words, ticks, _ = XO.expand(self.oracle, both, status, src, mv, self.actors, mode)
                out.append((src, mv, both, {k: v.copy() for k, v in status.items()}, words))
            return tuple(out)
        return self._once(("expand", mode), make)


class Frozen(MixedModel):
    """everything the API can read of a model at one moment (a copy of readable()), compared with a handle as the model itself is"""

    def __init__(self, model):   # (deliberately not the model's __init__: nothing is played on this)
        self.auto_reset = model.auto_reset
        self._r = {k: np.array(v, copy=True) for k, v in model.readable().items()}
        _frozen(*self._r.values())

    def readable(self):
        return self._r


_MATES = {}


def mates(oracle):
    """the one Mates of a test run (the CPU and the GPU module share it and what it has computed)"""
    if id(oracle) not in _MATES:
        _MATES[id(oracle)] = Mates(oracle)
    return _MATES[id(oracle)]
