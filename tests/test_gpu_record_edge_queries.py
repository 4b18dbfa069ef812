"""The search, reach and view calls at the limits of the packed record.  The directed corpus of tests/edge_states.py has so far met the
step kernels, the plain observation and the SimpleAgent policy only; every call below embeds the tick in a kernel of its own or reads the
record directly (pom_batch_step_mixed, the closed loop's call, among them: test_step_mixed), and has been fed hand-made cases of ordinary size and played games.  Here pom_batch_forecast, _move_safety, _rollout
(both forms), _rollout_jobs, _expand, _reach, _observe_view and _remember_view answer for (tests/edge_queries.py)
  A  the 1,337 uploadable states the corpus reaches at ticks 0, 1, 2, 3, 5, 8, 13, 24 and at each entry's end, with the moves its script
     plays next: 4,015 envs, every state in three tile columns, the last tile short;
  B  the 20 narrow-field entries played on a MODE_RAW handle for 26 ticks and asked after every tick (63 envs): fields beyond upload's
     bounds (bombCount -128, maxBombCount 32,655, bombStrength 141, aliveAgents -128) are reached only this way;
  C  10 hand-made states (31 envs): timeStep at the ends of int32, bomb words with every nibble at 15 and with the moved bit, queued
     flames with timeLeft 127 and -128, flagged flame cells 1 and 10 cells from their origins along all four rays, and two in which
     bombs, a flame and agents leave a viewer's window between the view memory's two calls.
Every comparison is byte-exact against the calls' checkers (tests/*_oracle.py), which sit on the oracle's Step; every expectation is
computed before the GPU is touched.  The CPU part says what the inputs reach, so that a change of the corpus is noticed.

Where a tick raises POM_UB_FLAME_QUEUE_RANGE the record holds a flame timeLeft at -128 or flames.count at 255 (pom_state.h): of a
downloaded State only the flame queue's bytes may then differ from the oracle's (expand's children, the tick of the view memory's test);
the calls' own outputs are compared in full."""
import functools

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE, is_flame
from tests import edge_queries as EQ
from tests import move_safety_oracle as MO
from tests import rollout_oracle as RO
from tests import view_oracle as VO
from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE, narrow_field_entries
from tests.mixed_model import MixedModel
from tests.test_emul import emul_bins  # noqa: F401  (the host builds of the device tick, built as test_emul.py builds them)
from tests.test_record_edges import _pack_roundtrip, assert_tick_matches

gpu = pytest.mark.gpu
SETS = ("A", "B", "C")
UPLOADED = ("A", "C")


@pytest.fixture(scope="module")
def sets(oracle):
    """sets(which) -> [Queries]: one batch for A and C; for B one per tick, the first one's states uploaded and the moves of each played to
    reach the next.  Built on first use and shared by the module's tests."""
    make = {"A": lambda: [EQ.set_a(oracle)], "B": lambda: EQ.set_b(oracle), "C": lambda: [EQ.set_c(oracle)]}
    return functools.lru_cache(maxsize=None)(lambda which: make[which]())


# ---------------------------------------------------------------------------------------------------------------- CPU: the inputs
def test_selection_is_what_the_module_says(oracle, sets):
    names, states, moves = EQ.selected_states(oracle)
    a = sets("A")[0]
    assert (states.size, a.d, a.n) == (1393, 1337, 4015)
    assert int((states["flames_count"] > 20).sum()) == 822 and int((a.states["flames_count"] > 20).sum()) == 822
    assert int((moves != 0).any(axis=1).sum()) == 86 and int((a.moves != 0).any(axis=1).sum()) == 62
    assert len(set(a.names)) == a.d and set(a.names) <= set(names)
    assert all(EQ.uploadable(s) for s in a.states) and sum(not EQ.uploadable(s) for s in states) == 1393 - 1337
    # what set A never holds, and set C is for
    live = np.arange(20)[None, :] < a.states["bombs_count"][:, None]
    bombs = np.take_along_axis(a.states["bombs_queue"], (a.states["bombs_index"][:, None] + np.arange(20)) % 20, axis=1).astype(np.int64)
    assert not a.states["timeStep"].any() and not ((bombs >> 20) & 0xFF)[live].any() and int(((bombs >> 16) & 0xF)[live].max()) == 10
    queued = np.arange(20)[None, :] < np.minimum(a.states["flames_count"], 20)[:, None]
    left = np.take_along_axis(a.states["flames_queue"]["timeLeft"], (a.states["flames_index"][:, None] + np.arange(20)) % 20, axis=1)
    assert int(left[queued].max()) == 4 and int(left[queued].min()) == -128


def test_played_entries_are_the_narrow_field_entries_without_a_flag(oracle, sets):
    b = sets("B")
    every = [e.name for e in narrow_field_entries()]
    names = [n.rsplit("@", 1)[0] for n in b[0].names]
    assert len(names) == 20 and set(every) - set(names) == {"flame_time_to_minus128"}
    lengths = [len(e.moves) for e in narrow_field_entries() if e.name in names]
    assert (min(lengths), max(lengths), len(b)) == (5, 26, 27) and b[0].n == 63
    beyond = {n for q in b for n, s in zip(names, q.states) if not EQ.uploadable(s)}
    assert len(beyond) == 10, sorted(beyond)
    fin = {n: s for n, s in zip(names, b[-1].states)}
    assert int(fin["bombcount_down_-108"]["agents"]["bombCount"][2]) == -128 and int(fin["alive_-124"]["aliveAgents"]) == -128
    assert max(int(q.states["agents"]["maxBombCount"].max()) for q in b) == 32655
    assert max(int(q.states["agents"]["bombStrength"].max()) for q in b) == 141
    # the states of tick t + 1 are the states of tick t after its moves, flag-free
    for q, nxt in zip(b, b[1:]):
        s = q.states.copy()
        assert not (oracle.step_batch(s, q.moves) & (FATAL | UB_FLAME_QUEUE_RANGE)).any()
        s["agents"]["pad"] = 0
        assert s.tobytes() == nxt.states.tobytes()


@pytest.mark.parametrize("which", SETS)
def test_placement_puts_every_state_into_several_columns(sets, which):
    for q in sets(which)[:1]:
        assert q.n % 16 == 15 and np.array_equal(q.order[0:3 * q.d:3], np.arange(q.d))
        cols, short = EQ.columns_of(q.order, q.d)
        assert all(len(c) >= 3 for c in cols) and set().union(*cols) == set(range(16)) and len(short) >= min(q.d, 5)
        assert all(q.order[q.env_of(j, r)] == j for j in range(q.d) for r in range(3))


def test_hand_states_hold_what_they_are_for_and_pass_upload(oracle, sets, emul_bins):  # noqa: F811
    import ctypes as C
    c = sets("C")[0]
    by = dict(zip(c.names, c.states))
    assert [int(by[f"timestep_{t}"]["timeStep"]) for t in (2**31 - 1, -1, -2**31)] == [2**31 - 1, -1, -2**31]
    words = by["bomb_nibbles_15_and_moved_bit"]["bombs_queue"][:3].astype(np.int64)
    assert int(by["bomb_nibbles_15_and_moved_bit"]["bombs_count"]) == 3
    assert ((words >> 12) & 0xFFF == 0xFFF).sum() == 1 and ((words >> 24) & 1).sum() == 2 and ((words >> 20) & 0xF).tolist() == [0, 4, 15]
    for t in (127, -128):
        s = by[f"flame_timeleft_{t}"]
        k = [int(v) for v in s["flames_queue"]["timeLeft"][:2]].index(t)
        f = s["flames_queue"][k]
        assert int(s["flames_count"]) == 2 and int(s["board"][f["y"], f["x"]]) == (4 << 16) + ((int(f["x"]) + 11 * int(f["y"])) << 3)
    seen = set()
    for name, rays in (("flagged_rays_x", (0, 1)), ("flagged_rays_y", (2, 3))):
        s = by[name]
        board = s["board"].astype(np.int64)
        for y, x in zip(*np.nonzero(is_flame(board) & (board & 7 != 0))):
            origin, flag = (int(board[y, x]) & 0xFFFF) >> 3, int(board[y, x]) & 7
            oy, ox = divmod(origin, 11)
            ray, dist = (0 if x > ox else 1, abs(x - ox)) if oy == y else (2 if y > oy else 3, abs(y - oy))
            beside = [a for a in s["agents"] if not a["dead"] and abs(int(a["x"]) - x) + abs(int(a["y"]) - y) == 1]
            assert ray in rays and beside and (ox == x or oy == y)
            seen.add((ray, dist, flag))
    assert {(r, d) for r, d, _ in seen} == {(r, d) for r in range(4) for d in (1, 10)} and {f for _, _, f in seen} == {1, 2, 3}
    # upload takes each (pom_step's packer: pom_pack_state's field widths and the live-bomb rule), and the device tick body, built for
    # the host one lane and four lanes per env, plays each as the oracle does: the state's own moves, then 11 ticks standing still
    run = emul_bins.pom_emul_run
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    run.restype = C.c_int
    T = 12
    for name, s, mv in zip(c.names, c.states, c.moves):
        s = s.reshape(1).copy()
        assert _pack_roundtrip(emul_bins, s.copy(), "pom_step") == 0, f"{name}: upload refuses it"
        moves = np.zeros((T, 4), dtype=np.int32)
        moves[0] = mv
        want, want_ubs, o = np.zeros((T, 1004), dtype=np.uint8), np.zeros(T, dtype=np.uint32), s.copy()
        for t in range(T):
            want_ubs[t] = oracle.step(o, moves[t])
            o["agents"]["pad"] = 0
            want[t] = np.frombuffer(o.tobytes(), dtype=np.uint8)
        for quad in (0, 1):
            got, ubs = np.zeros((T, 1004), dtype=np.uint8), np.zeros(T, dtype=np.uint32)
            assert run(s.ctypes.data, moves.ctypes.data, T, quad, got.ctypes.data, ubs.ctypes.data) == 0, name
            for t in range(T):
                assert_tick_matches(f"{name} (quad {quad})", t, want, want_ubs, got[t].tobytes(), ubs[t])
    assert all(_pack_roundtrip(emul_bins, s.reshape(1).copy(), "pom_step") == 0 for s in sets("A")[0].states[::9])


def test_the_corpus_states_make_the_search_calls_answer_both_ways(sets):
    """conditions on set A (counts measured when this was written, over its 1,337 states: 67 agents die within the forecast, 40 are dead
    at the start, 300 candidate moves end in a death and 53 in a walker with nowhere to stand)"""
    a = sets("A")[0]
    flame, agent, ub = a.forecast(True)
    flags = int(np.bitwise_or.reduce(ub))
    assert flags & 0x27 == 0x27, hex(flags)           # LOST_AGENT, NULL_BOMB, QUEUE_OVERFLOW, FLAME_QUEUE_RANGE
    assert (agent > 0).any() and (agent == -1).any() and (agent == 0).any()
    assert (flame == 0).any() and int(flame.max()) > 7 and int(agent.max()) > 7      # (the prefixes below cut something off)
    for h in EQ.FORECAST_PREFIXES:
        f_h, a_h, ub_h = a.forecast(True, h)
        assert int(f_h.max()) <= h and int(a_h.max()) <= h and (ub_h & ~ub == 0).all() and (ub_h != ub).any()
    death, escape = a.move_safety(False)
    assert (death > 0).any() and (escape > 0).any() and (death == -1).any() and (death == 0).any()
    d2, e2 = a.move_safety(True)
    assert (d2[:, [1, 3]] == MO.UNASKED).all() and (d2[:, [0, 2]] != MO.UNASKED).all() and (d2 > 0).any() and (e2 > 0).any()
    for words in (a.rollout(RO.DIST_RANDOM, False), a.rollout(RO.DIST_STRESS, True), a.rollout_policy(), a.jobs()[2]):
        for bit in (RO.RO_UB, RO.RO_DONE):
            assert (words & bit != 0).any() and (words & bit == 0).any(), hex(bit)
        assert (words >> RO.RO_LENGTH_SHIFT).max() > 1
    src, mv, _ = a.jobs()
    assert len(src) == a.d + len(range(0, a.d, 5)) and len(set(src.tolist())) == len(src) and len(set(a.order[src].tolist())) == a.d
    for mode in (0, 1):
        src, want, status, words = a.expand(mode)
        assert (words & RO.RO_UB != 0).any() and (status["ubflags"][a.n:] & FATAL != 0).any() and (status["ubflags"][a.n:] & UB_FLAME_QUEUE_RANGE != 0).any()
        assert want[:a.n].tobytes() == a.placed.tobytes()


def test_viewer_attrs_reach_the_record_fields_bounds(sets):
    attrs, alive = [], []
    for q in sets("A") + sets("B"):
        attrs.append(q.viewer_attrs())
        alive.append(q.observed()[2][:, 1])
    va, alive = np.concatenate(attrs), np.concatenate(alive)
    assert va[:, :, 4].min() <= -108 and va[:, :, 4].max() >= 107          # bombCount
    assert va[:, :, 5].min() == -32768 and va[:, :, 5].max() >= 32646      # maxBombCount
    assert va[:, :, 6].max() >= 134 and alive.min() < 0                     # bombStrength; env_attrs' aliveAgents
    assert va[:, :, 4].min() == -128 and va[:, :, 5].max() == 32655 and va[:, :, 6].max() == 141 and alive.min() == -128   # (set B)
    planes = np.concatenate([q.view_planes("uint8") for q in sets("A")])
    assert int(planes[:, :, 12].max()) == 15                                # plane 12, a bomb's strength nibble


def test_reach_floods_past_flagged_flames_and_bombs(sets):
    """a living agent with a flagged flame cell (record codes 136..255) beside a cell it reaches, and one with a bomb there"""
    found = {"flagged": 0, "bomb": 0, "flame": 0}
    for q in sets("A") + sets("C"):
        dist, _ = q.reach()
        board = q.states["board"].astype(np.int64)
        kinds = {"flagged": is_flame(board) & (board & 7 != 0), "bomb": board == 3, "flame": is_flame(board)}
        ag = q.states["agents"]
        reached = dist > 0
        e, v = np.nonzero(ag["dead"] == 0)
        reached[e, v, ag["y"][e, v], ag["x"][e, v]] = True
        beside = MO.grow(reached, np.ones((1, 1, 11, 11), dtype=bool)) & ~reached
        for k, m in kinds.items():
            found[k] += int((beside & m[:, None]).any(axis=(2, 3)).sum())
    assert all(found.values()), found


@pytest.mark.parametrize("radius", [1, 4])
def test_fog_has_flames_and_bombs_on_both_sides_of_a_window(sets, radius):
    a = sets("A")[0]
    codes, attrs, _ = a.observed()
    w = VO.windows(attrs, radius)
    for name, code in (("bomb", 3), ("flame", 4)):
        m = np.broadcast_to(codes[:, None, 0] == code, w.shape)
        assert (m & w).any() and (m & ~w).any(), name
    assert (attrs[:, :, 2] == 0).any() and int(codes[:, 4].max()) == 4 and (a.view_codes(radius)[:, :, 0] == VO.FOG).any()


def test_the_memory_ages_bombs_flames_and_agents_between_the_two_calls(sets):
    """the view memory's own rule (pom_batch.h PomMemorySpec 1.2 - 1.4) has something to do at the second call of test_remember_view:
    cells seen at the first call and outside the window at the second (age 1) that held a ticking bomb — the time nibble at 15 among them
    —, a bomb that runs out, a flame remembered with life 127, an agent that stays remembered on its bomb, one seen elsewhere that gives
    way to the bomb it stood on, and one that died.  Set A alone ages 51 cells, none of them with anything on it: set C's leaves_window
    states are there for this."""
    from tests.view_memory_oracle import AGE, BOARD, BOMB, FLAME, FLAMES, LIFE
    c = sets("C")[0]
    (m0, _), after, _ = c.memory()
    m1, _ = c.memory_after(after)
    for name in ("leaves_window_x", "leaves_window_y"):
        j = c.names.index(name)
        was, now = m0[j, 0].astype(int), m1[j, 0].astype(int)             # agent 0's view
        aged = (was[AGE] == 0) & (now[AGE] == 1)
        assert aged.sum() == 9, name                                       # the column (row) that left the window
        assert ((was[LIFE] == 15) & (now[LIFE] == 14) & (now[BOARD] == BOMB) & aged).sum() == 1, name
        assert ((was[LIFE] == 1) & (was[BOARD] == BOMB) & (now[LIFE] == 0) & (now[BOARD] == 0) & aged).sum() == 1, name
        assert ((was[BOARD] == FLAMES) & (was[FLAME] == 127) & (now[BOARD] == FLAMES) & (now[FLAME] == 126) & aged).sum() == 1, name
        assert ((was[BOARD] == 11) & (was[LIFE] == 9) & (now[BOARD] == 11) & (now[LIFE] == 8) & aged).sum() == 1, name     # agent 1 stays
        assert ((was[BOARD] == 12) & (was[LIFE] == 5) & (now[BOARD] == BOMB) & (now[LIFE] == 4) & aged).sum() == 1, name   # agent 2 seen elsewhere
        assert ((was[BOARD] == 13) & (now[BOARD] == 0) & aged).sum() == 1 and after["agents"]["dead"][j, 3], name          # agent 3 died
    a = sets("A")[0]
    (a0, _), a_after, _ = a.memory()
    a1, _ = a.memory_after(a_after)
    aged = (a0[:, :, AGE] == 0) & (a1[:, :, AGE] == 1)
    assert aged.sum() == 51 and not (aged & ((a0[:, :, LIFE] > 0) | (a0[:, :, BOARD] == FLAMES) | (a0[:, :, BOARD] >= 10))).any()


# ---------------------------------------------------------------------------------------------------------------- GPU
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _same(q, what, got, want, env_axis=0):
    """got (a device tensor or an array, the placed batch's) against want, byte for byte; a difference is named by its state"""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    if got.dtype != want.dtype:
        assert got.dtype.itemsize == want.dtype.itemsize, (what, got.dtype, want.dtype)
        got = got.view(want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{what}: {len(bad)} values differ in {len(set(bad[:, env_axis].tolist()))} envs, first at {bad[0].tolist()} = "
                           f"{q.name_of_env(bad[0][env_axis])}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}")


def _walk(qs, check):
    """the first batch uploaded; each batch asked where the record stands on it (B: after the moves of the one before were played, the
    downloaded States the oracle's byte for byte); the calls leave the batch as it is"""
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    with BatchEnvironment(qs[0].n, mode=MODE_RAW) as env:
        env.make_game(qs[0].placed)
        for t, q in enumerate(qs):
            if t:
                env.step(qs[t - 1].placed_moves)
            assert env.get_state().tobytes() == q.placed.tobytes(), f"tick {t}: the record is not the oracle's state"
            check(env, q, f"tick {t}")
            assert env.get_state().tobytes() == q.placed.tobytes(), f"tick {t}: a call changed the batch"
            assert not env.status()["ubflags"].any() or len(qs) == 1


@gpu
@pytest.mark.parametrize("which", SETS)
def test_forecast(hip_lib, sets, which):
    """horizon 32 with the states' next moves and standing still; horizons 1 and 7 are its prefixes, their flags a run of their own"""
    qs = sets(which)
    for q in qs:
        for with_moves in (True, False):
            for h in (EQ.FORECAST_K,) + EQ.FORECAST_PREFIXES:
                q.forecast(with_moves, h)

    def check(env, q, what):
        mv = _dev(q.placed_moves)
        for with_moves in (True, False):
            for h in (EQ.FORECAST_K,) + EQ.FORECAST_PREFIXES:
                got = env.forecast(h, moves=mv if with_moves else None, ubflags=True)
                for name, want in zip(("flame_tick", "agent_tick", "ubflags"), q.forecast(with_moves, h)):
                    _same(q, f"{what}, horizon {h}, moves {with_moves}: {name}", got[name], want[q.order])
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("which", SETS)
def test_move_safety(hip_lib, sets, which):
    """horizon 10: all agents, the others standing still; agents 0 and 2 with the states' next moves as the others' moves"""
    qs = sets(which)
    for q in qs:
        q.move_safety(False), q.move_safety(True)

    def check(env, q, what):
        got = env.move_safety(EQ.SAFETY_K)
        for name, want in zip(("death_tick", "escape_tick"), q.move_safety(False)):
            _same(q, f"{what}, all agents: {name}", got[name], want[q.order])
        got = env.move_safety(EQ.SAFETY_K, agents=EQ.SAFETY_MASK, moves=_dev(q.placed_moves))
        for name, want in zip(("death_tick", "escape_tick"), q.move_safety(True)):
            want = np.where(want == MO.UNASKED, -1, want)[q.order]   # rows not asked for: -1 in a tensor the call allocates
            _same(q, f"{what}, agents {EQ.SAFETY_MASK:#x}: {name}", got[name], want)
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("which", SETS)
def test_rollout(hip_lib, sets, which):
    """horizon 24, 2 samples: DIST_RANDOM, and DIST_STRESS after the states' next moves as tick 1"""
    qs = sets(which)
    for q in qs:
        q.rollout(RO.DIST_RANDOM, False), q.rollout(RO.DIST_STRESS, True)

    def check(env, q, what):
        got = env.rollout(EQ.ROLLOUT_K, EQ.ROLLOUT_R, EQ.SEED, RO.DIST_RANDOM)
        _same(q, f"{what}, DIST_RANDOM", got, q.rollout(RO.DIST_RANDOM, False), env_axis=1)
        got = env.rollout(EQ.ROLLOUT_K, EQ.ROLLOUT_R, EQ.SEED, RO.DIST_STRESS, moves=_dev(q.placed_moves))
        _same(q, f"{what}, DIST_STRESS after the next moves", got, q.rollout(RO.DIST_STRESS, True), env_axis=1)
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("which", SETS)
def test_rollout_policy(hip_lib, sets, which):
    """horizon 12, 1 sample, fresh SimpleAgents in seats 1 and 3, for every env of the batch (4,015 of set A: the checker takes 2 s)"""
    qs = sets(which)
    for q in qs:
        q.rollout_policy()

    def check(env, q, what):
        got = env.rollout(EQ.POLICY_K, EQ.POLICY_R, EQ.SEED, RO.DIST_RANDOM, simple=EQ.POLICY_MASK, fresh_agents=True)
        _same(q, f"{what}, simple {EQ.POLICY_MASK:#x}", got, q.rollout_policy(), env_axis=1)
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("which", SETS)
def test_rollout_jobs(hip_lib, sets, which):
    """every distinct state once, every fifth twice (other envs, other moves), shuffled: horizon 24, 2 samples, DIST_STRESS after the
    jobs' moves, agent 2 a SimpleAgent"""
    qs = sets(which)
    for q in qs:
        q.jobs()

    def check(env, q, what):
        src, mv, want = q.jobs()
        got = env.rollout_jobs(_dev(src), EQ.ROLLOUT_K, EQ.ROLLOUT_R, EQ.SEED, RO.DIST_STRESS, moves=_dev(mv), simple=EQ.JOBS_SIMPLE, first=0xF,
                               fresh_agents=True)
        got = got.cpu().numpy().view(np.uint32)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} words differ, first job {bad[0].tolist()} = {q.name_of_env(src[bad[0][1]])}: got {got[tuple(bad[0])]:#x}, want {want[tuple(bad[0])]:#x}"
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("mode", [0, 1], ids=["raw", "env"])
@pytest.mark.parametrize("which", UPLOADED)
def test_expand(hip_lib, sets, which, mode):
    """every distinct state, from one of its envs, into a slot behind the batch with its next moves — the ticks that raise fatal flags
    among them: words, children, statuses and flags are the checker's, the sources are left alone"""
    from pomcpp_amd.batch import BatchEnvironment
    q = sets(which)[0]
    src, want, status, want_words = q.expand(mode)
    with BatchEnvironment(q.n + q.d, mode=mode, auto_reset=False) as env:
        env.make_game(np.concatenate([q.placed, np.zeros(q.d, dtype=STATE_DTYPE)]))
        words = env.expand(src, q.moves, first=q.n).cpu().numpy().view(np.uint32)
        got, st = env.get_state(), env.status()
    bad = np.nonzero(words != want_words)[0]
    assert bad.size == 0, f"{len(bad)} words differ, first {q.names[bad[0]]}: got {words[bad[0]]:#x}, want {want_words[bad[0]]:#x}"
    assert got[:q.n].tobytes() == q.placed.tobytes(), "a source changed"
    g, w = got.view(np.uint8).reshape(-1, 1004), want.view(np.uint8).reshape(-1, 1004)
    held = (status["ubflags"] & UB_FLAME_QUEUE_RANGE) != 0
    differs = (g != w)
    differs[held, EQ.QUEUE_BYTES] = False                     # pom_state.h: the record holds the queue at -128 / 255
    bad = np.nonzero(differs.any(axis=1))[0]
    assert bad.size == 0, f"{len(bad)} children differ, first {q.names[bad[0] - q.n]}: bytes {np.nonzero(differs[bad[0]])[0][:12].tolist()}"
    assert (got["flames_count"][held] == np.minimum(want["flames_count"][held], 255)).all()
    assert (got["flames_queue"]["timeLeft"][held] >= -128).all() and held[q.n:].any() and not held[:q.n].any()
    for k in ("done", "winner", "draw", "ubflags"):
        bad = np.nonzero(st[k] != status[k])[0]
        assert bad.size == 0, f"status {k}: {len(bad)} differ, first env {bad[0]}: got {st[k][bad[0]]}, want {status[k][bad[0]]}"


@gpu
@pytest.mark.parametrize("which", SETS)
def test_reach(hip_lib, sets, which):
    qs = sets(which)
    for q in qs:
        q.reach()

    def check(env, q, what):
        got = env.reach(max_dist=120)
        for name, want in zip(("dist", "move"), q.reach()):
            _same(q, f"{what}: {name}", got[name], want[q.order])
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("which", SETS)
def test_code_views(hip_lib, sets, which):
    """radii 0, 1, 4 and 10: the code planes, viewer_attrs (sign-extended agent fields) and env_attrs' timeStep and aliveAgents"""
    qs = sets(which)
    want = [{r: q.view_codes(r) for r in EQ.RADII} for q in qs]
    for q in qs:
        q.viewer_attrs()

    def check(env, q, what):
        for r in EQ.RADII:
            got, vattrs, eattrs = env.observe(dtype="codes", view_radius=r)
            _same(q, f"{what}, radius {r}: codes", got, want[qs.index(q)][r][q.order])
            _same(q, f"{what}, radius {r}: viewer_attrs", vattrs, q.viewer_attrs()[q.order])
            _same(q, f"{what}, radius {r}: env_attrs", eattrs[:, :2], q.observed()[2][q.order])
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("dtype", EQ.PLANE_DTYPES)
@pytest.mark.parametrize("which", SETS)
def test_plane_views(hip_lib, sets, which, dtype):
    """radius 4, the 16 planes in all three element types"""
    qs = sets(which)
    want = [q.view_planes(dtype) for q in qs]
    for q in qs:
        q.viewer_attrs()

    def check(env, q, what):
        got, vattrs, eattrs = env.observe(dtype=dtype, view_radius=EQ.PLANE_RADIUS)
        _same(q, f"{what}, {dtype} planes", got, want[qs.index(q)][q.order])
        _same(q, f"{what}, {dtype}: viewer_attrs", vattrs, q.viewer_attrs()[q.order])
        _same(q, f"{what}, {dtype}: env_attrs", eattrs[:, :2], q.observed()[2][q.order])
    _walk(qs, check)


@gpu
@pytest.mark.parametrize("which", UPLOADED)
def test_remember_view(hip_lib, sets, which):
    """a MODE_ENV handle without auto-reset: a call from a wiped memory, one tick of step_device with the states' next moves, a second
    call; radius 4, all four views, every env of the batch (4,015 of set A: the checker takes 1.4 s).

    A tick that raises FLAME_QUEUE_RANGE leaves a flame queue in the record that is not the reference's (pom_state.h: timeLeft held at
    -128, count at 255; the next flame then goes to another slot), and the remembered flame life is read off that queue.  For those
    states (81 of set A, 1 of set C) the second call's expectation is computed on the oracle's State with the record's queue bytes in it,
    as downloaded after the tick; every other byte of the State, and every other state's expectation, is the oracle's from before the GPU
    is touched."""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import MODE_ENV, RESET_OFF, BatchEnvironment
    q = sets(which)[0]
    (m0, s0), after, ub = q.memory()
    m1, s1 = q.memory_after(after)
    held = np.nonzero(ub & UB_FLAME_QUEUE_RANGE)[0]
    assert 0 < held.size <= q.d // 8
    with BatchEnvironment(q.n, mode=MODE_ENV, auto_reset=RESET_OFF) as env:
        env.make_game(q.placed)
        assert not env.episodes().any()
        memory, stamp = pa.new_view_memory(q.n)
        env.remember(memory, stamp, EQ.MEMORY_RADIUS, EQ.MEMORY_MASK)
        env.sync()
        _same(q, "call 0: memory", memory, m0[q.order])
        _same(q, "call 0: stamp", stamp, s0[q.order])
        env.step_device(_dev(q.placed_moves))
        env.sync()
        got, st = env.get_state(), env.status()
        _same(q, "the tick's flags", st["ubflags"].astype(np.uint32), ub[q.order])
        g = got.view(np.uint8).reshape(-1, 1004)
        differs = g != after[q.order].view(np.uint8).reshape(-1, 1004)
        differs[np.isin(q.order, held), EQ.QUEUE_BYTES] = False
        assert not differs.any(), f"the tick: first {q.name_of_env(np.nonzero(differs.any(axis=1))[0][0])}"
        record = after[held].copy()
        for i, j in enumerate(held):
            envs = [q.env_of(j, r) for r in range(3)]
            assert (g[envs] == g[envs[0]]).all(), f"{q.names[j]}: its three envs hold different records after the tick"
            record[i:i + 1].view(np.uint8)[EQ.QUEUE_BYTES] = g[envs[0], EQ.QUEUE_BYTES]
        m1, s1 = m1.copy(), s1.copy()
        m1[held], s1[held] = q.memory_after(record, held)
        env.remember(memory, stamp, EQ.MEMORY_RADIUS, EQ.MEMORY_MASK)
        env.sync()
        _same(q, "call 1: memory", memory, m1[q.order])
        _same(q, "call 1: stamp", stamp, s1[q.order])


# ---------------------------------------------------------------------------------------------------------------- pom_batch_step_mixed
MIXED_MASKS = (0, 0b1010, 0xF)
MIXED_RADIUS = 4
MIXED_HELD = {"A": 245, "C": 3}                       # envs whose tick raises FLAME_QUEUE_RANGE, under every mask (81 states of A, 1 of C)
MIXED_FATAL = {"A": {0: 9, 0b1010: 9, 0xF: 0}}         # envs whose tick raises a fatal flag: compared in full


class _RawTicks:
    """MixedModel (tests/mixed_model.py) for a MODE_RAW handle: Environment::Step's bookkeeping left out, the tick alone"""

    def __init__(self, oracle):
        self.simple_policy, self.boardgen, self._step = oracle.simple_policy, oracle.boardgen, oracle.step

    def env_step(self, state, moves, status):
        return self._step(state, moves)


def _mixed_views(states):
    ob = EQ.observe_oracle()
    _, attrs, env2 = ob.observe(states)
    return VO.view_codes(ob.observe_codes(states), attrs, MIXED_RADIUS), VO.viewer_attrs(attrs, env2[:, 0]), env2


def _mixed_outputs(n):
    import torch
    out = (torch.full((n, 4, 5, 11, 11), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((n, 4, 12), -7, dtype=torch.int32, device="cuda"),
           torch.full((n, 4), -7, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()   # the sentinels are in place before the handle's stream writes
    return out


def _mixed_matches(q, what, env, model, outs, first, count, env0=0):
    """envs [first, first + count) of the handle after ONE mixed tick against the model's: state, status, flags, memory, and the fused
    fogged codes.  An env whose tick raised FLAME_QUEUE_RANGE may differ in EQ.QUEUE_BYTES only (assert_tick_matches' exemption); its
    views are then the oracles' of the model's State with the record's queue bytes in it (as test_remember_view).  -> envs held"""
    rows = slice(first, first + count)
    got, st = env.get_state()[rows], env.status()
    want = model.states[rows].copy()
    held = (model.ubflags[rows] & UB_FLAME_QUEUE_RANGE) != 0
    g, w = got.view(np.uint8).reshape(-1, 1004), want.view(np.uint8).reshape(-1, 1004)
    differs = g != w
    differs[held, EQ.QUEUE_BYTES] = False
    bad = np.nonzero(differs.any(axis=1))[0]
    assert bad.size == 0, f"{what}: {len(bad)} states differ, first {q.name_of_env(env0 + bad[0])}: bytes {np.nonzero(differs[bad[0]])[0][:12].tolist()}"
    assert (got["flames_count"][held] == np.minimum(want["flames_count"][held], 255)).all() and (got["flames_queue"]["timeLeft"][held] >= -128).all()
    for k, mine in (("done", model.done), ("winner", model.winner), ("draw", model.draw), ("ubflags", model.ubflags)):
        _same(q, f"{what}: status {k}", np.asarray(st[k][rows]).astype(mine.dtype), mine[rows])
    _same(q, f"{what}: memory", env.policy_memory()[rows], model.mems[rows])
    w[held, EQ.QUEUE_BYTES] = g[held, EQ.QUEUE_BYTES]
    for name, got_t, want_a in zip(("codes", "viewer_attrs", "env_attrs"), outs, _mixed_views(want)):
        got_a = got_t.cpu().numpy()[rows]
        _same(q, f"{what}: fused fogged {name}", got_a[:, :2] if name == "env_attrs" else got_a, want_a)
    return held


@gpu
@pytest.mark.parametrize("which", SETS)
def test_step_mixed(hip_lib, oracle, sets, which):
    """one tick of pom_batch_step_mixed on every state with its next moves: the scripts alone (mask 0), SimpleAgents in seats 1 and 3, and
    in all four — fresh agents, seed EQ.SEED, the fused fogged codes of radius 4 — against tests/mixed_model.py.  A and C: a MODE_ENV
    handle per mask.  B: the MODE_RAW handle that plays the entries holds every env a second time behind the batch; after every tick of
    the walk the records are copied there (copy_envs: the record as it stands, fields beyond upload's bounds included) and ticked once
    under each mask, the model's tick being Oracle.step alone."""
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW, RESET_OFF, BatchEnvironment
    qs = sets(which)
    if which in UPLOADED:
        q = qs[0]
        models = {}
        for mask in MIXED_MASKS:
            models[mask] = MixedModel(oracle, q.placed)
            models[mask].tick_mixed(0, q.n, q.placed_moves, mask, EQ.SEED, 0)
        for mask in MIXED_MASKS:
            with BatchEnvironment(q.n, mode=MODE_ENV, auto_reset=RESET_OFF) as env:
                env.make_game(q.placed)
                env.sync()
                outs = _mixed_outputs(q.n)
                env.step_mixed(0, q.n, _dev(q.placed_moves), mask, EQ.SEED, 0, None, codes=outs[0], view_radius=MIXED_RADIUS, viewer_attrs=outs[1],
                               env_attrs=outs[2])
                env.sync()
                held = _mixed_matches(q, f"mask {mask:#x}", env, models[mask], outs, 0, q.n)
                assert int(held.sum()) == MIXED_HELD[which] and 0 < len(set(q.order[held].tolist())) <= q.d // 8
                fatal = (models[mask].ubflags & FATAL) != 0
                assert int(fatal.sum()) == MIXED_FATAL.get(which, {}).get(mask, 0)
                assert np.array_equal(env.counters(), models[mask].counters)
        return
    n = qs[0].n
    back = n + (-n) % 16                                 # the copies start on a tile of their own
    raw = _RawTicks(oracle)
    models = []                                          # [tick][mask]: the model of the whole handle, its second part ticked once
    for t, q in enumerate(qs):
        both = np.concatenate([q.placed, np.zeros(back - n, dtype=STATE_DTYPE), q.placed])
        mv = np.concatenate([q.placed_moves, np.zeros((back - n, 4), dtype=np.int32), q.placed_moves])
        row = {}
        for mask in MIXED_MASKS:
            row[mask] = MixedModel(raw, both)
            row[mask].tick_mixed(back, n, mv, mask, EQ.SEED, t)
        models.append((mv, row))
    asked = 0
    with BatchEnvironment(back + n, mode=MODE_RAW) as env:
        env.make_game(np.concatenate([qs[0].placed, np.zeros(back - n + n, dtype=STATE_DTYPE)]))
        env.step_mixed(0, 0, None, 0xF, EQ.SEED, 0)   # (allocates the agents' memory: copy_envs then copies the walk's fresh agents)
        outs = _mixed_outputs(back + n)
        for t, q in enumerate(qs):
            if t:
                env.step_mixed(0, back, _dev(models[t - 1][0]), 0, EQ.SEED, t - 1)   # the walk itself: the scripts through the mixed kernel
                env.sync()
            assert env.get_state(0, n).tobytes() == q.placed.tobytes(), f"tick {t}: the record is not the oracle's state"
            mv, row = models[t]
            for mask in MIXED_MASKS:
                env.copy_envs(np.arange(n, dtype=np.int64), first=back)
                env.step_mixed(back, n, _dev(mv), mask, EQ.SEED, t, None, codes=outs[0], view_radius=MIXED_RADIUS, viewer_attrs=outs[1], env_attrs=outs[2])
                env.sync()
                _mixed_matches(q, f"tick {t}, mask {mask:#x}", env, row[mask], outs, back, n)
                asked += int(row[mask].mems[back:].any(axis=(1, 2)).sum())
            assert env.get_state(0, n).tobytes() == q.placed.tobytes(), f"tick {t}: the copies' ticks changed the batch"
    assert asked > len(qs) * n   # SimpleAgents were asked on the states beyond upload's bounds too
