"""The visits a launch waits for: long chained blasts (explode_long's look / commit / nest / way back, the removal of several bombs
from the middle of the queue in one tick) and wavefronts that restart several envs in one visit (restart_columns: up to four
snapshot records per round with their loads in flight together).

Chains: hand-made states of strength-3 bombs in some columns of a wavefront, beside mates that do short blasts, choose their bombs
in loop B or do nothing (the actors of tests/tile_mates.py).  What a state claims — how deep it nests, that a look meets a cell whose
bomb has left the queue — is asserted on the CPU, through the instrumented host builds of the device tick and the oracle, before the
GPU is asked anything.  Restarts: 1, 2, 4, 5 and all 16 envs of a tile finish on one tick.  Every tick is compared with the oracle."""
import ctypes as C

import numpy as np
import pytest

import pomcpp_amd as pa
import pomcpp_amd.state as S
from pomcpp_amd.state import STATE_DTYPE, Item
from tests import tile_mates as TM
from tests.edge_states import Entry, _base, _idle
from tests.test_emul import emul_bins  # noqa: F401  (the host builds of the device body)

T = 4            # ticks every chain actor is played: the blast on tick 0, its flames until they go out
SIZES = (16, 17, 37)
P_MAXFRAME, P_MASK = 0, 1   # tests/emul/pom_emul_probe.h, as tests/test_tile_mates.py reads it
PROBE_WORDS = 8 + TM.LAYOUT["stack_depth"]


# ---------------------------------------------------------------------------------------------------------------- the chain actors
def _bombs(cells, strength=3, first_life=1):
    """strength-3 bombs on `cells` in queue order, the head about to time out (TickBombs sets it off on tick 0)"""
    s = _base()
    TM._bombers(s, 30, strength)
    for k, (x, y) in enumerate(cells):
        S.plant_bomb(s[0], x, y, k % 4, set_item=True, life_time=first_life if k == 0 else 10)
    assert int(s["bombs_count"][0]) == len(cells)
    return s


LINE = [(1, 5), (3, 5), (5, 5), (7, 5), (9, 5), (9, 7)]
CROSS = [(5, 5), (7, 5), (9, 5), (9, 7), (9, 9), (3, 5), (1, 5), (5, 7), (5, 3), (5, 1)]
GRID = [(x, y) for r, y in enumerate((1, 3, 5, 7)) for x in ((1, 3, 5, 7, 9) if r % 2 == 0 else (9, 7, 5, 3, 1))]


def chain_actors():
    out = []
    # a line: every blast's ray meets the next bomb two cells on; the last but one turns the corner.  The last blast's +y ray ends ON
    # wood (9, 9), its +x ray in front of rigid (10, 7)
    s = _bombs(LINE)
    s["board"][0, 9, 9] = Item.WOOD
    s["board"][0, 7, 10] = Item.RIGID
    out.append((Entry("line_wood_rigid", s, _idle(T), "six bombs in a line, the chain ends on wood and on rigid"), 5))
    # the same line with agent 1 standing on the third bomb (the cell shows the agent, the bomb is queued under him)
    s = _bombs(LINE)
    s["board"][0, 0, 10] = Item.PASSAGE
    S.put_agent(s[0], 5, 5, 1)
    out.append((Entry("line_agent_on_bomb", s, _idle(T), "an agent stands on a chained bomb"), 5))
    # a cross: the centre's four rays each meet a bomb; the +x arm goes on round the corner, four frames deep
    out.append((Entry("cross", _bombs(CROSS), _idle(T), "a cross of ten bombs, its longest arm four frames deep"), 4))
    # a full queue: 20 bombs on a grid two cells apart, all set off by the head in one tick — 19 removals from inside the queue
    out.append((Entry("grid20", _bombs(GRID), _idle(T), "a full queue, every bomb but the head removed from inside it"), 4))
    # the same with the queue's head wrapped round the end of the ring
    s = _base()
    s["bombs_index"] = 13
    TM._bombers(s, 30, 3)
    for k, (x, y) in enumerate(GRID):
        S.plant_bomb(s[0], x, y, k % 4, set_item=True, life_time=1 if k == 0 else 10)
    out.append((Entry("grid20_idx13", s, _idle(T), "a full queue that starts at slot 13"), 4))
    # the set of bomb cells is too large: queue T (5,5), Y (9,5), X (7,5), Z (3,5).  T sets off X (offset 2), X sets off Y (offset 1,
    # removed first), so X's own removal at its stale offset 2 takes Z out of the queue instead — Z never goes off and
    # its cell still shows BOMB when T's -x ray gets there: in the set, not in the queue, struck, looked at again
    out.append((Entry("struck_cell", _bombs([(5, 5), (9, 5), (7, 5), (3, 5)]), _idle(T), "a look settles on a cell whose bomb has left the queue"), 2))
    return out


class Stage:
    def __init__(self, oracle):
        mine = chain_actors()
        self.depth = {e.name: d for e, d in mine}
        self.entries = [e for e, _ in mine] + TM.actors(oracle)
        for e in self.entries:
            e.start["agents"]["pad"] = 0
        self.ix = {e.name: i for i, e in enumerate(self.entries)}
        self.states, self.ubs = TM.solo_traces(oracle, self.entries, ticks=T)
        self.sticky = np.bitwise_or.accumulate(self.ubs, axis=1)
        self.chains = [e.name for e, _ in mine]
        # the company: short blasts (strength-1 chains set off by the head: deep_top), bombs chosen in loop B (select, claims_full,
        # a strength-1 chain set off inside loop B), a bounce, and nothing at all
        self.mates = ["deep_top_d2", "select_c63", "quiet_idle", "claims_full", "deep_b_rest_d5", "bounce_4", "quiet_all_dead", "select1_c63"]

    def who(self, n):
        """a chain actor in every other column, each at several columns, the mates between them"""
        names = []
        for c in range(n):
            names.append(self.chains[(c // 2 + c // 16) % len(self.chains)] if c % 2 == 0 else self.mates[(c // 2) % len(self.mates)])
        return np.array([self.ix[k] for k in names], dtype=np.int32)


@pytest.fixture(scope="module")
def stage(oracle):
    return Stage(oracle)


def _probe(lib, e, quad):
    run = lib.pom_emul_run_probe
    run.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    run.restype = C.c_int
    got, ubs = np.zeros((T, 1004), dtype=np.uint8), np.zeros(T, dtype=np.uint32)
    probe = np.zeros((T, PROBE_WORDS), dtype=np.int32)
    mv = np.ascontiguousarray(e.moves, dtype=np.int32)
    assert run(e.start.ctypes.data, mv.ctypes.data, T, quad, got.ctypes.data, ubs.ctypes.data, probe.ctypes.data) == 0, e.name
    return got, ubs, probe


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("quad", [0, 1], ids=["one_lane", "quad"])
def test_chain_actors_reach_what_they_are_for(emul_bins, stage, quad):  # noqa: F811
    """the host build of the device tick agrees with the oracle on every tick of every chain actor, and its frame probe shows the
    nesting each actor claims; the states themselves show the rest"""
    for name in stage.chains:
        i = stage.ix[name]
        e = stage.entries[i]
        got, ubs, pr = _probe(emul_bins, e, quad)
        assert not (ubs & 0x40000000).any(), f"{name}: the quad model's checks failed"
        assert np.array_equal(ubs, stage.ubs[i]) and np.array_equal(got, stage.states[i]), name
        d = stage.depth[name]
        assert pr[0, P_MAXFRAME] >= d - 1 and pr[0, P_MASK] & ((1 << d) - 1) == (1 << d) - 1, (name, pr[0, :8].tolist())
        assert int(e.start["agents"]["bombStrength"][0].min()) >= 3
    after = lambda name: stage.states[stage.ix[name], 0].view(STATE_DTYPE)[0]  # noqa: E731
    assert stage.depth["line_wood_rigid"] >= 4 and stage.depth["cross"] >= 4
    s = after("line_wood_rigid")
    assert int(s["bombs_count"]) == 0 and S.is_flame(s["board"][9, 9]) and int(s["board"][7, 10]) == Item.RIGID
    s = after("line_agent_on_bomb")
    assert int(s["agents"][1]["dead"]) == 1 and int(s["aliveAgents"]) == 3 and int(s["bombs_count"]) == 0
    assert int(after("cross")["bombs_count"]) == 0
    for name in ("grid20", "grid20_idx13"):
        e = stage.entries[stage.ix[name]]
        assert int(e.start["bombs_count"][0]) == 20 and int(after(name)["bombs_count"]) == 0  # 19 removals from inside the queue
    # struck_cell.  The host builds have no counter inside explode_long (the probe counts at the store interface, and a struck cell
    # is a look that writes nothing), so that the look-again path ran is shown by what only it can leave behind:
    #  - when the tick began Z was queued on (3, 5) and its cell showed BOMB: the set of bomb cells, built at the tick's first long
    #    blast from the whole queue, holds (3, 5);
    #  - Z never went off: three flames were spawned, at T, X and Y, none at (3, 5) — yet Z has left the queue, whose one remaining
    #    word is X's ghost;
    #  - T's -x ray, looked at after X's blast had returned, went THROUGH (3, 5) and on to (2, 5): the look stopped at a BOMB cell of
    #    the set, found no bomb for it in the queue, struck it and looked again — a look that trusted the set would have nested there
    #    (a fourth flame), one that skipped the cell's test would have done so on tick 0 of every other chain actor too.
    e = stage.entries[stage.ix["struck_cell"]]
    z = int(e.start["bombs_queue"][0, 3])
    assert (z & 0xF, (z >> 4) & 0xF) == (3, 5) and int(e.start["bombs_count"][0]) == 4 and int(e.start["board"][0, 5, 3]) == Item.BOMB
    s = after("struck_cell")
    assert int(s["flames_count"]) == 3 and int(s["bombs_count"]) == 1
    origins = {(int(f["x"]), int(f["y"])) for f in s["flames_queue"][:3]} if int(s["flames_index"]) == 0 else None
    assert origins == {(5, 5), (7, 5), (9, 5)}, origins
    left = int(s["bombs_queue"][int(s["bombs_index"])])
    assert (left & 0xF, (left >> 4) & 0xF) == (7, 5)
    assert S.is_flame(s["board"][5, 3]) and S.is_flame(s["board"][5, 2])


# ---------------------------------------------------------------------------------------------------------------- GPU: chains
def _check(stage, who, t, got_states, got_ubs, what):
    n = who.size
    g = got_states.view(np.uint8).reshape(n, 1004)
    w = stage.states[who, t]
    bad = np.nonzero((g != w).any(axis=1) | (np.asarray(got_ubs, dtype=np.uint32) != stage.sticky[who, t]))[0]
    assert bad.size == 0, (f"{what}: env {bad[0]} (column {bad[0] % 16}) actor {stage.entries[who[bad[0]]].name} tick {t}: bytes "
                           f"{np.nonzero(g[bad[0]] != w[bad[0]])[0][:12].tolist()} differ; {bad.size} envs in all")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_chains_plain_one_tick_kernel(hip_lib, stage, n):
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    who = stage.who(n)
    start, moves = TM.batch(stage.entries, who, ticks=T)
    with BatchEnvironment(n, mode=MODE_RAW) as env:
        env.make_game(start)
        for t in range(T):
            env.step(moves[t])
            _check(stage, who, t, env.get_state(), env.status()["ubflags"], "plain")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_chains_chained_kernel_two_calls_back_to_back(hip_lib, stage, n):
    import torch
    from pomcpp_amd.batch import ISSUE_CHAIN, MODE_RAW, BatchEnvironment
    who = stage.who(n)
    start, moves = TM.batch(stage.entries, who, ticks=T)
    tape = torch.from_numpy(moves).to("cuda:0")
    for pieces in ((1, 1, 1, 1), (2, 2)):
        with BatchEnvironment(n, mode=MODE_RAW, issue_mode=ISSUE_CHAIN) as env:
            assert env.issue_info()[0] == "chain"
            env.make_game(start)
            t = 0
            for k in range(0, len(pieces), 2):  # two calls, then a look
                for piece in pieces[k:k + 2]:
                    env.step_device_many(tape[t:t + piece].contiguous())
                    t += piece
                env.sync()
                _check(stage, who, t - 1, env.get_state(), env.status()["ubflags"], f"chained {pieces}")
            assert env.chain_stats()["tiles_recovered"] == 0


def _solo_env_runs(oracle, stage, cap):
    """every actor alone under Environment::Step with its script, restarting from its start state when its game ends (what the
    end-of-tick reset shows): states [A, T, 1004] as shown after each tick, finished [A, T]"""
    A = len(stage.entries)
    shown, fin = np.zeros((A, T, 1004), dtype=np.uint8), np.zeros((A, T), dtype=bool)
    for i, e in enumerate(stage.entries):
        s, st = e.start.copy(), dict(done=0, winner=-1, draw=0)
        for t in range(T):
            oracle.env_step(s, e.moves[t], st)
            if st["done"] or int(s["timeStep"][0]) >= cap:
                fin[i, t] = True
                s, st = e.start.copy(), dict(done=0, winner=-1, draw=0)
            s["agents"]["pad"] = 0
            shown[i, t] = np.frombuffer(s.tobytes(), dtype=np.uint8)
    return shown, fin


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_chains_reset_at_end(hip_lib, oracle, stage, n):
    """explicit moves, POM_RESET_AT_END: a game a chain finishes (quiet_all_dead at once) is back on its start state after the tick"""
    from pomcpp_amd.batch import CNT_EPISODES, CNT_RESETS, CNT_STEPS, MODE_ENV, RESET_AT_END, BatchEnvironment
    cap = 800
    shown, fin = _solo_env_runs(oracle, stage, cap)
    who = stage.who(n)
    start, moves = TM.batch(stage.entries, who, ticks=T)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=cap) as env:
        env.make_game(start)
        for t in range(T):
            env.step(moves[t])
            g = env.get_state().view(np.uint8).reshape(n, 1004)
            bad = np.nonzero((g != shown[who, t]).any(axis=1))[0]
            assert bad.size == 0, f"tick {t}: env {bad[0]} actor {stage.entries[who[bad[0]]].name}"
            assert env.last_results()["finished"].astype(bool).tolist() == fin[who, t].tolist(), t
        cnt = env.counters()
    assert cnt[CNT_STEPS] == n * T and cnt[CNT_EPISODES] == cnt[CNT_RESETS] == int(fin[who].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_chains_four_ticks_per_launch(hip_lib, oracle, stage, n):
    """the tile stays in LDS between the ticks of a launch: the same start states under the random move stream (the chains go off
    on tick 0 whatever the agents in the corners do), against the oracle's run of the batch after every launch"""
    from pomcpp_amd.batch import DIST_RANDOM, MODE_ENV, BatchEnvironment
    who, seed = stage.who(n), 23
    start, _ = TM.batch(stage.entries, who, ticks=T)
    ref = start.copy()
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(start)
        for k in range(3):
            env.step_random(seed, DIST_RANDOM, ticks=4, ticks_per_launch=4)
            oracle.run_random(ref, start, 4, seed, 0, 4 * k, DIST_RANDOM, 800)
            want = ref.copy()
            want["agents"]["pad"] = 0
            assert env.get_state().tobytes() == want.tobytes(), f"after tick {4 * k + 3}"


# ---------------------------------------------------------------------------------------------------------------- GPU: restarts
def _bytes(states):
    w = states.copy()
    w["agents"]["pad"] = 0
    return w.tobytes()


CAP = 5
FINISHING = (1, 2, 4, 5, 16)


def _restart_start(n, k):
    """n boards; in tile 0, k envs (spread over the tile, both ends included from k = 2 on) one tick from the step cap; the tiles
    after it get k - 1 and k + 1 such envs (mod 17), so that no two tiles of a batch restart alike"""
    start = pa.make_boards(n, seed=40 + k)
    start["agents"]["pad"] = 0
    for tile in range((n + 15) // 16):
        kk = (k + (0, 16, 1)[tile % 3]) % 17
        cols = sorted({(j * 15) // max(kk - 1, 1) for j in range(kk)}) if kk > 1 else [7]
        cols = cols if len(cols) == kk else list(range(kk))
        for c in cols:
            if tile * 16 + c < n:
                start["timeStep"][tile * 16 + c] = CAP - 1
    return start


@pytest.mark.gpu
@pytest.mark.parametrize("issue", ["plain", "chained"])
@pytest.mark.parametrize("n", SIZES)
def test_restarts_at_start_from_the_snapshot(hip_lib, oracle, n, issue):
    from pomcpp_amd.batch import (CNT_EPISODES, CNT_RESETS, CNT_STEPS, DIST_RANDOM, ISSUE_AUTO, ISSUE_CHAIN, MODE_ENV, RESET_AT_START,
                                  BatchEnvironment)
    seed, ticks = 5, 2 * CAP + 2
    for k in FINISHING:
        start = _restart_start(n, k)
        assert int((start["timeStep"][:16] == CAP - 1).sum()) == k
        ref = start.copy()
        finished = restarts = 0
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=CAP,
                              issue_mode=ISSUE_CHAIN if issue == "chained" else ISSUE_AUTO) as env:
            env.make_game(start)
            for t in range(ticks):
                restarts += int(((ref["aliveAgents"] <= 1) | (ref["timeStep"] >= CAP)).sum())
                oracle.run_random(ref, start, 1, seed, 0, t, DIST_RANDOM, CAP)
                done = (ref["aliveAgents"] <= 1) | (ref["timeStep"] >= CAP)
                finished += int(done.sum())
                env.step_random(seed, DIST_RANDOM, ticks=1)
                assert env.get_state().tobytes() == _bytes(ref), f"k {k} tick {t}"
                assert env.status()["done"].astype(bool).tolist() == done.tolist(), (k, t)
            cnt = env.counters()
        assert restarts >= 2 * k and cnt[CNT_STEPS] == n * ticks and cnt[CNT_EPISODES] == finished and cnt[CNT_RESETS] == restarts, (k, cnt)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_restarts_at_end_with_terminal_records(hip_lib, oracle, n):
    from pomcpp_amd.batch import CNT_EPISODES, CNT_RESETS, CNT_STEPS, DIST_RANDOM, MODE_ENV, RESET_AT_END, BatchEnvironment
    seed, ticks = 5, 2 * CAP + 2
    for k in FINISHING:
        start = _restart_start(n, k)
        ref, term = start.copy(), np.zeros(n, dtype=start.dtype)
        finished = 0
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=CAP) as env:
            env.make_game(start)
            for t in range(ticks):
                oracle.run_random(ref, start, 1, seed, 0, t, DIST_RANDOM, CAP)  # (restarts whoever the tick before left finished)
                done = (ref["aliveAgents"] <= 1) | (ref["timeStep"] >= CAP)
                finished += int(done.sum())
                term[done] = ref[done]
                env.step_random(seed, DIST_RANDOM, ticks=1)
                want = ref.copy()
                want[done] = start[done]
                assert env.get_state().tobytes() == _bytes(want), f"k {k} tick {t}"
                assert env.last_results()["finished"].astype(bool).tolist() == done.tolist(), (k, t)
                assert env.get_terminal_state()[done].tobytes() == _bytes(term[done]), (k, t)
                assert not env.status()["done"].any()
            cnt = env.counters()
        assert finished >= 2 * k and cnt[CNT_STEPS] == n * ticks and cnt[CNT_EPISODES] == cnt[CNT_RESETS] == finished, (k, cnt)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_restarts_in_the_two_kernel_policy_path(hip_lib, oracle, n):
    """policy_simple judges a restarting env on the board it restarts on (the policy kernel's own restart from the snapshot),
    step_policy then restarts it for good: states and the agents' memory against the oracle's SimpleAgent run"""
    from pomcpp_amd.batch import CNT_EPISODES, CNT_RESETS, CNT_STEPS, MODE_ENV, RESET_AT_START, BatchEnvironment
    seed, ticks = 9, 2 * CAP + 2
    for k in FINISHING:
        start = _restart_start(n, k)
        ref, mems = start.copy(), np.zeros((n, 4, 16), dtype=np.int32)
        finished = restarts = 0
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=CAP) as env:
            env.make_game(start)
            for t in range(ticks):
                restarts += int(((ref["aliveAgents"] <= 1) | (ref["timeStep"] >= CAP)).sum())
                oracle.run_simple(ref, start, mems, 1, seed, 0, t, CAP)
                finished += int(((ref["aliveAgents"] <= 1) | (ref["timeStep"] >= CAP)).sum())
                env.policy_simple(seed)
                env.step_policy()
                assert env.get_state().tobytes() == _bytes(ref), f"k {k} tick {t}"
                assert np.array_equal(env.policy_memory(), mems), (k, t)
            cnt = env.counters()
        assert cnt[CNT_STEPS] == n * ticks and cnt[CNT_EPISODES] == finished and cnt[CNT_RESETS] == restarts, (k, cnt)
