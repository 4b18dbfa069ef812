"""TEST INFRASTRUCTURE — the record-edge corpus (tests/edge_states.py) as inputs of the calls that embed the tick in a kernel of their own
or read the record directly: forecast, move_safety, the rollouts, expand, reach, the fogged views and the view memory.  Numpy only, no GPU:
the inputs, where each sits in a batch, and what every call must answer, all from checkers that restate nothing of a kernel
(tests/*_oracle.py on the oracle's Step, which tests/golden/edge_cases.npz pins to the compiled reference on this very corpus).

Three kinds of input:
  A  states the corpus reaches and upload accepts: of every entry the states after 0, 1, 2, 3, 5, 8, 13 and 24 scripted ticks and its
     last one, each with the moves its entry's script plays next;
  B  the narrow-field entries played on the device, tick by tick, so that the record holds fields beyond upload's bounds;
  C  hand-made states for what the corpus never holds (hand_states()).
A Queries object holds the distinct states of one batch with their next moves, the placement of tests/test_record_edges._batch — state i
at env 3i, states i + 7 and i + 13 beside it, a short tail to 15 mod 16 — and computes every checker once per distinct state; the rows
are gathered by the placement (`order`).  The rollouts' draws are keyed by the env, so their checkers run on the placed batch.
Queries(..., order=) takes another placement — any int array naming the state of every env, tests/mates_queries.py passes the chosen
wavefronts of tests/tile_mates.py —: env_of(), jobs() and expand() then speak of "an env that holds state j", and of the states the
order holds at all."""
import functools
import importlib.util
import os

import numpy as np

import pomcpp_amd.state as S
from pomcpp_amd.state import STATE_DTYPE, Item
from tests import expand_oracle as XO
from tests import forecast_oracle as FO
from tests import move_safety_oracle as MO
from tests import reach_cases as RC
from tests import rollout_jobs_oracle as JO
from tests import rollout_oracle as RO
from tests import rollout_policy_oracle as PO
from tests import view_memory_oracle as VM
from tests import view_oracle as VO
from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE, corpus, narrow_field_entries, uploadable  # noqa: F401  (uploadable: for callers)
from tests.policy_edge_states import edge_corpus_states

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICKS = (0, 1, 2, 3, 5, 8, 13, 24)                       # of every entry, and its last state
QUEUE_BYTES = slice(STATE_DTYPE.fields["flames_queue"][1], 1004)   # flames.queue, flames.index, flames.count: the tail of the State
SEED = 20261021
FORECAST_K, FORECAST_PREFIXES = 32, (1, 7)
SAFETY_K, SAFETY_MASK = 10, 0b0101
ROLLOUT_K, ROLLOUT_R = 24, 2
POLICY_K, POLICY_R, POLICY_MASK = 12, 1, 0b1010
JOBS_SIMPLE = 0b0100                                     # the jobs' playouts: agent 2 plays SimpleAgent after the given tick-1 moves
RADII, PLANE_RADIUS, PLANE_DTYPES = (0, 1, 4, 10), 4, ("uint8", "float16", "float32")
MEMORY_RADIUS, MEMORY_MASK = 4, 15


@functools.lru_cache(maxsize=None)
def observe_oracle():
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def placement(d):
    """test_record_edges._batch's order for d distinct states: i, i + 7, i + 13 for every i, then the first states again until the batch
    size is 15 mod 16 — every state sits in several tile columns, some in the last, partial tile"""
    order = [j for i in range(d) for j in (i, (i + 7) % d, (i + 13) % d)]
    order += [k % d for k in range((15 - len(order)) % 16)]
    assert len(order) % 16 == 15
    return np.array(order, dtype=np.int64)


def columns_of(order, d):
    """[{tile columns}] per distinct state, and the states of the last, partial tile"""
    cols = [set() for _ in range(d)]
    for k, j in enumerate(order):
        cols[int(j)].add(k % 16)
    return cols, set(order[len(order) - len(order) % 16:].tolist())


# ---------------------------------------------------------------------------------------------------------------- the inputs
def _script_row(entry, tick):
    return entry.moves[tick] if tick < len(entry.moves) else np.zeros(4, dtype=np.int32)


def selected_states(oracle):
    """set A before upload's bounds are asked: (names, states STATE_DTYPE[N], moves int32[N, 4]) — of every corpus entry the states
    `entry@tick` of tests/policy_edge_states.edge_corpus_states for the ticks of TICKS and its last one, each with the row of the
    entry's script that is played next (IDLE past its end)"""
    entries = {e.name: e for e in corpus(oracle)}
    by_entry = {}
    for name, s in edge_corpus_states(oracle):
        entry, tick = name.rsplit("@", 1)
        by_entry.setdefault(entry, []).append((int(tick), s))
    names, states, moves = [], [], []
    for entry, run in by_entry.items():
        last = run[-1][0]
        for tick, s in run:
            if tick in TICKS or tick == last:
                names.append(f"{entry}@{tick}")
                states.append(s)
                moves.append(_script_row(entries[entry], tick))
    return names, np.concatenate(states), np.array(moves, dtype=np.int32).reshape(-1, 4)


def played_entries(oracle):
    """set B: the narrow-field entries whose whole oracle run raises neither a fatal flag nor FLAME_QUEUE_RANGE, and the number of ticks
    of the longest (shorter scripts are padded with IDLE, which raises neither flag either: asserted)"""
    out = []
    ticks = max(len(e.moves) for e in narrow_field_entries())
    for e in narrow_field_entries():
        e.start["agents"]["pad"] = 0
        s, ub = e.start.copy(), 0
        for t in range(len(e.moves)):
            ub |= oracle.step(s, e.moves[t])
        if ub & (FATAL | UB_FLAME_QUEUE_RANGE):
            continue
        for t in range(len(e.moves), ticks):
            assert not oracle.step(s, np.zeros(4, dtype=np.int32)) & (FATAL | UB_FLAME_QUEUE_RANGE), e.name
        out.append(e)
    return out, ticks


def _flame(s, x, y, time_left, strength, flag=0, origin=None):
    """a flame cell; with `origin` None also its queue entry (entries are appended: the caller keeps timeLeft ascending)"""
    ox, oy = (x, y) if origin is None else origin
    s["board"][0, y, x] = Item.FLAMES + ((ox + 11 * oy) << 3) + flag
    if origin is None:
        k = int(s["flames_count"][0])
        s["flames_queue"][0, k] = (x, y, time_left, strength)
        s["flames_count"][0] = k + 1


def _corners():
    s = S.new_states(1)
    S.put_agents_in_corners(s[0])
    return s


def _busy(time_step):
    """a board on which something happens within a few ticks: two bombs, one about to go off, a flame, wood beside it"""
    s = _corners()
    s["timeStep"][0] = time_step
    s["agents"]["maxBombCount"][0] = 3
    S.plant_bomb(s[0], 0, 2, 0, set_item=True, life_time=2)
    S.plant_bomb(s[0], 8, 10, 3, set_item=True, life_time=6)
    s["board"][0, 3, 0] = Item.WOOD + 1
    _flame(s, 5, 5, 2, 1)
    return s


def _flagged(vertical):
    """flagged flame cells 10 cells and 1 cell from their origins along +x and -x (vertical: +y and -y), flags 1..3, each beside a living
    agent; the origins are queued, the rays' cells between origin and end burn too"""
    s = S.new_states(1)
    at = (lambda x, y: (y, x)) if vertical else (lambda x, y: (x, y))
    flags = (2, 3, 1, 3) if vertical else (1, 2, 3, 1)
    rays = [((3, 6), (4, 6), 1, 3, flags[2]), ((7, 8), (6, 8), 1, 3, flags[3]),      # 1 cell along +x, along -x
            ((0, 1), (10, 1), 10, 4, flags[0]), ((10, 3), (0, 3), 10, 4, flags[1])]   # 10 cells along +x, along -x
    for (ox, oy), (ex, ey), strength, time_left, flag in rays:
        _flame(s, *at(ox, oy), time_left, strength)
        step = 1 if ex > ox else -1
        for x in range(ox + step, ex, step):
            _flame(s, *at(x, oy), 0, 0, origin=at(ox, oy))
        _flame(s, *at(ex, ey), 0, 0, flag=flag, origin=at(ox, oy))
    for i, (x, y) in enumerate(((10, 2), (0, 2), (4, 7), (6, 7))):   # beside (10, 1) and (10, 3); (0, 1) and (0, 3); (4, 6); (6, 8)
        S.put_agent(s[0], *at(x, y), i)
    return s


def _leaves_window(vertical):
    """for the view memory's own rule: agent 0 at (4, 5) sees, in column 8 — the edge of its radius-4 window —, a bomb word with strength
    and time nibbles at 15, a bomb with one tick left, a flame with timeLeft 127, agent 1 standing on its bomb, agent 2 standing on its
    bomb and agent 3 beside the flame; its move takes it to (3, 5), so all of column 8 is remembered, not seen, at the next call.
    Meanwhile agent 1 stays (its code is kept, its bomb counts down), agent 2 steps into agent 0's new window (its remembered code
    gives way to the bomb it stood on) and agent 3 steps into the flame and dies (its remembered code gives way to passage).
    vertical: the same with x and y exchanged.  -> (state, moves)"""
    s = S.new_states(1)
    at = (lambda x, y: (y, x)) if vertical else (lambda x, y: (x, y))
    for i, (x, y) in enumerate(((4, 5), (8, 7), (8, 6), (8, 2))):
        S.put_agent(s[0], *at(x, y), i)
    s["agents"]["maxBombCount"][0] = 3
    s["agents"]["bombStrength"][0, 3] = 0                # (the bomb that goes off this tick burns its own cell only)
    bombs = ((8, 8, 3, 0, 1), (8, 6, 2, 1, 5), (8, 7, 1, 1, 9), (8, 5, 3, 15, 15))   # x, y, owner, strength, time: timers ascending
    for k, (x, y, owner, strength, time) in enumerate(bombs):
        x, y = at(x, y)
        s["bombs_queue"][0, k] = S._i32(x | (y << 4) | (owner << 8) | (strength << 12) | (time << 16))
        if s["board"][0, y, x] < Item.AGENT0:
            s["board"][0, y, x] = Item.BOMB
        s["agents"]["bombCount"][0, owner] += 1
    s["bombs_count"][0] = len(bombs)
    _flame(s, *at(8, 3), 127, 0)
    I, U, D, L, R = 0, 1, 2, 3, 4
    return s, ((U, I, U, R) if vertical else (L, I, L, D))


def hand_states():
    """set C: [(name, state, moves)] — what set A never holds (timeStep is 0 there, bomb direction 0, bomb life at most 10, flame timeLeft
    at most 4).  The queued flames with timeLeft 127 and -128 are two states: pom_state.h promises board and agents past
    FLAME_QUEUE_RANGE (which -128 raises on the first tick) only while every queued timeLeft is <= 4.  The two leaves_window states
    give the view memory's countdown and stale-agent rules something to do (set A's scripts hardly move a window)."""
    I, U, D, L, R, B = 0, 1, 2, 3, 4, 5
    out = [(f"timestep_{t}", _busy(t), (D, B, U, L)) for t in (2**31 - 1, -1, -2**31)]
    s = _corners()                                        # live bomb words: the moved bit (1 << 24) set, every nibble at 15; timers ascending
    s["agents"]["maxBombCount"][0] = 4
    words = ((0, 4, 2, (3 << 12) | (1 << 16) | (1 << 24)), (6, 10, 3, (2 << 12) | (5 << 16) | (4 << 20) | (1 << 24)),
             (4, 0, 0, (15 << 12) | (15 << 16) | (15 << 20)))
    for k, (x, y, owner, word) in enumerate(words):
        s["bombs_queue"][0, k] = S._i32(x | (y << 4) | (owner << 8) | word)
        s["board"][0, y, x] = Item.BOMB
        s["agents"]["bombCount"][0, owner] += 1
    s["bombs_count"][0] = 3
    out.append(("bomb_nibbles_15_and_moved_bit", s, (R, I, I, B)))
    for t in (127, -128):                                 # a queued flame at an end of the record's signed byte, seen on the board
        s = _corners()
        for x, y, time_left, strength in sorted(((2, 0, 2, 1), (5, 5, t, 2)), key=lambda f: f[2]):
            _flame(s, x, y, time_left, strength)
        _flame(s, 6, 5, 0, 0, origin=(5, 5))
        s["board"][0, 6, 5] = Item.WOOD + 2
        out.append((f"flame_timeleft_{t}", s, (R, I, I, U)))
    out.append(("flagged_rays_x", _flagged(False), (U, D, U, D)))
    out.append(("flagged_rays_y", _flagged(True), (L, R, L, R)))
    out.append(("leaves_window_x", *_leaves_window(False)))
    out.append(("leaves_window_y", *_leaves_window(True)))
    for _, s, _ in out:
        s["agents"]["pad"] = 0
    return [(n, s, np.array(m, dtype=np.int32)) for n, s, m in out]


# ---------------------------------------------------------------------------------------------------------------- the expectations
class Queries:
    """the distinct states of one batch, the moves each plays next, the placement, and every checker's answer (computed on first use,
    kept, never written again)"""

    def __init__(self, oracle, names, states, moves, order=None):
        self.oracle, self.names = oracle, list(names)
        self.states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        self.moves = np.ascontiguousarray(moves, dtype=np.int32).reshape(-1, 4)
        self.d = self.states.size
        assert len(self.names) == self.d == len(self.moves)
        self.order = placement(self.d) if order is None else np.array(order, dtype=np.int64)
        assert self.order.ndim == 1 and self.order.size and 0 <= self.order.min() and self.order.max() < self.d
        self.n = len(self.order)
        # a given order: the envs of every state, in the batch's order, and the states it holds (the default holds every state thrice)
        self._envs = None if order is None else [np.nonzero(self.order == j)[0] for j in range(self.d)]
        self.held = np.arange(self.d) if order is None else np.unique(self.order)
        self.placed, self.placed_moves = self.states[self.order], self.moves[self.order]
        self._kept = {}

    def _once(self, key, make):
        if key not in self._kept:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._kept[key] = v
        return self._kept[key]

    def env_of(self, j, r):
        """the env that holds state j as the r-th of its triple (r = 0, 1, 2: i, i + 7, i + 13); under a given order: an env that holds
        state j, the r-th of them (counted round)"""
        if self._envs is not None:
            return int(self._envs[j][r % len(self._envs[j])])
        return 3 * ((j - (0, 7, 13)[r]) % self.d) + r

    def name_of_env(self, k):
        return f"{self.names[int(self.order[k])]} (env {k})"

    # ---- forecast: (flame_tick, agent_tick, ubflags) per distinct state
    def forecast(self, with_moves, horizon=FORECAST_K):
        if horizon == FORECAST_K:
            return self._once(("forecast", with_moves), lambda: FO.forecast(self.oracle, self.states, horizon, self.moves if with_moves else None))
        # a shorter horizon is a prefix: what happens after its last tick has not happened; the flags come from a run of their own
        flame, agent, _ = self.forecast(with_moves)
        ub = self._once(("forecast_ub", with_moves, horizon),
                        lambda: FO.forecast(self.oracle, self.states, horizon, self.moves if with_moves else None)[2])
        return np.where(flame > horizon, 0, flame).astype(np.uint8), np.where(agent > horizon, 0, agent).astype(np.int32), ub

    # ---- move_safety: (death_tick, escape_tick) per distinct state; rows not asked for are MO.UNASKED
    def move_safety(self, masked):
        agents = [a for a in range(4) if SAFETY_MASK >> a & 1] if masked else [0, 1, 2, 3]
        return self._once(("safety", masked), lambda: MO.move_safety(self.oracle, self.states, SAFETY_K, self.moves if masked else None, agents))

    # ---- rollouts: result words of the PLACED batch (the draws are keyed by the env)
    def rollout(self, dist, with_moves):
        return self._once(("rollout", dist, with_moves), lambda: RO.rollout(self.oracle, self.placed, ROLLOUT_K, ROLLOUT_R, SEED, dist,
                                                                            self.placed_moves if with_moves else None))

    def rollout_policy(self):
        """fresh SimpleAgents in the seats of POLICY_MASK, the others draw: uint32 [POLICY_R, n]"""
        return self._once("policy", lambda: PO.rollout(self.oracle, self.placed, None, POLICY_K, POLICY_R, SEED, RO.DIST_RANDOM, POLICY_MASK))

    def jobs(self):
        """a source list that names every distinct state once (at one of its three envs, by turns) and every fifth a second time at
        another, in a fixed shuffled order; the moves of a job: its state's next moves, for the second naming all BOMB.
        -> (src int64 [m], moves int32 [m, 4], words uint32 [ROLLOUT_R, m])"""
        first = np.array([self.env_of(j, j % 3) for j in self.held], dtype=np.int64)
        again = np.array([self.env_of(j, (j + 1) % 3) for j in self.held[::5]], dtype=np.int64)
        src = np.concatenate([first, again])
        mv = np.concatenate([self.moves[self.held], np.full((len(again), 4), 5, dtype=np.int32)])
        assert np.array_equal(self.order[first], self.held) and np.array_equal(self.order[again], self.held[::5])
        perm = np.random.default_rng(7).permutation(len(src))
        src, mv = src[perm], np.ascontiguousarray(mv[perm])
        words = self._once("jobs", lambda: JO.rollout_jobs(self.oracle, self.placed, None, src, ROLLOUT_K, ROLLOUT_R, SEED, RO.DIST_STRESS, JOBS_SIMPLE,
                                                           0xF, mv))
        return src, mv, words

    # ---- expand: env n + j becomes the child of one env of state j under the state's next moves
    def expand(self, mode):
        """-> (src int64 [d], the whole batch of n + d states after the call, its statuses, words, FLAME_QUEUE_RANGE raised per child);
        under a given order d counts the states it holds"""
        src = np.array([self.env_of(j, (j + 2) % 3) for j in self.held], dtype=np.int64)
        assert np.array_equal(self.order[src], self.held)

        def make():
            both = np.concatenate([self.placed, np.zeros(len(src), dtype=STATE_DTYPE)])
            want, status, words, ticks, _ = XO.expand(self.oracle, both, None, src, self.moves[self.held], self.n, mode)
            assert ticks == len(src)
            return want, status, words
        return (src,) + self._once(("expand", mode), make)

    # ---- reach: (dist, move) uint8 [d, 4, 11, 11]
    def reach(self):
        return self._once("reach", lambda: RC.expected_planes(self.states, *RC.fill_rmap(self.oracle, self.states)))

    # ---- the unfogged export of the distinct states, what the views and the memory are derived from
    def observed(self, states=None):
        def make(states=states):
            states = self.states if states is None else states
            ob = observe_oracle()
            _, attrs, env2 = ob.observe(states)
            return ob.observe_codes(states), attrs, env2
        return make() if states is not None else self._once("observed", make)

    def view_codes(self, radius):
        codes, attrs, _ = self.observed()
        return VO.view_codes(codes, attrs, radius)

    def view_planes(self, dtype):
        _, attrs, _ = self.observed()
        planes, _, _ = observe_oracle().observe(self.states, per_agent=True, dtype=getattr(np, dtype))
        return VO.view_planes(planes, attrs, PLANE_RADIUS)

    def viewer_attrs(self):
        _, attrs, env2 = self.observed()
        return VO.viewer_attrs(attrs, env2[:, 0])

    # ---- the view memory: a call from a wiped memory, one tick of Environment::Step with the next moves, a second call
    def memory(self):
        """-> (memory, stamp) after the first call, the states after the tick, the tick's flags; per distinct state"""
        def make():
            after, ub = self.states.copy(), np.zeros(self.d, dtype=np.uint32)
            for j in range(self.d):
                ub[j] = self.oracle.env_step(after[j:j + 1], self.moves[j], dict(done=0, winner=-1, draw=0))
            after["agents"]["pad"] = 0
            return self._remember(*VM.new_memory(self.d), self.states) + (after, ub)
        m0, s0, after, ub = self._once("memory", make)
        return (m0, s0), after, ub

    def memory_after(self, after, rows=None):
        """-> (memory, stamp) after the second call, on the states `after` the tick; rows: of these distinct states only (all)"""
        (m0, s0), _, _ = self.memory()
        rows = np.arange(self.d) if rows is None else rows
        return self._remember(m0[rows].copy(), s0[rows].copy(), after)

    def _remember(self, m, st, states):
        codes, attrs, env2 = self.observed(states)
        env = np.zeros((len(states), 4), dtype=np.int32)
        env[:, :2] = env2
        VM.remember(m, st, codes, attrs, env, np.zeros(len(states), dtype=np.uint32), MEMORY_RADIUS, MEMORY_MASK)
        return m, st


def set_a(oracle):
    names, states, moves = selected_states(oracle)
    keep = [k for k in range(states.size) if uploadable(states[k])]
    return Queries(oracle, [names[k] for k in keep], states[keep], moves[keep])


def set_b(oracle):
    """[Queries after 0, 1, ... ticks]: the first one's placed states are uploaded, and tick t plays placed_moves of Queries t"""
    entries, ticks = played_entries(oracle)
    names = [e.name for e in entries]
    moves = np.zeros((ticks + 1, len(entries), 4), dtype=np.int32)
    for k, e in enumerate(entries):
        moves[:len(e.moves), k] = e.moves
    s = np.concatenate([e.start for e in entries])
    out = []
    for t in range(ticks + 1):
        out.append(Queries(oracle, [f"{n}@{t}" for n in names], s.copy(), moves[t]))
        if t < ticks:
            oracle.step_batch(s, moves[t])
            s["agents"]["pad"] = 0
    return out


def set_c(oracle):
    names, states, moves = zip(*hand_states())
    return Queries(oracle, names, np.concatenate(states), np.array(moves))
