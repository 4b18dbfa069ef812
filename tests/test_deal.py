"""pom_batch_deal on the GPU (include/pom_batch.h PomDealSpec) against its checker (tests/deal_oracle.py): the boards, words and game
counters byte for byte; what a call must leave alone; the restart snapshot seen through restore(); the closed loop in which every game
starts on a new board, against the host model of the range step (tests/range_model.py) whose snapshots the checker refills."""
import ctypes as C

import numpy as np
import pytest

from tests import deal_oracle as DO
from tests.range_model import RangeModel

pytestmark = pytest.mark.gpu
SEED = 77


class Boards:
    """the checker's boards, each computed once"""

    def __init__(self, seed=SEED, layout=DO.STANDARD, env_offset=0):
        self.seed, self.layout, self.env_offset, self.cache = seed, layout, env_offset, {}

    def __call__(self, e, g):
        key = (int(e), int(g))
        if key not in self.cache:
            s, w = DO.deal(self.seed, key[0], key[1], self.layout, self.env_offset)
            self.cache[key] = s[0].copy(), w
        return self.cache[key]

    def many(self, envs, games):
        from pomcpp_amd.state import STATE_DTYPE
        states, words = np.zeros(len(envs), dtype=STATE_DTYPE), np.zeros(len(envs), dtype=np.uint32)
        for j, (e, g) in enumerate(zip(envs, games)):
            states[j], words[j] = self(e, g)
        return states, words


@pytest.fixture(scope="module")
def boards():
    return Boards()


def _everything(env, at_end=False):
    """all a deal must leave alone where it deals nothing: records, status, SimpleAgent memory, episodes, counters and, on a
    RESET_AT_END handle (`at_end`), the last finished episodes' results and terminal records"""
    out = dict(state=env.get_state(), memory=env.policy_memory(), episodes=env.episodes(), counters=env.counters())
    out.update({"status_" + k: v for k, v in env.status().items()})
    if at_end:
        out.update(terminal=env.get_terminal_state(), **{"last_" + k: v for k, v in env.last_results().items()})
    return out


def _snapshots(env):
    """the restart snapshots, seen through restore() on a copy of nothing: the states are put back afterwards by the caller's own means"""
    env.restore(np.ones(env.n, dtype=bool))
    return env.get_state()


@pytest.mark.parametrize("n,offset", [(5, 0), (16, 0), (37, 1000), (200, 0)])
def test_start_all_deals_the_checkers_boards_and_they_play(hip_lib, oracle, n, offset):
    import torch
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    cap, seed = 30, 5
    want, want_words = Boards(env_offset=offset).many(range(n), [0] * n)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=cap, env_offset=offset) as env:
        env.make_game(pa.make_boards(n, seed=3))
        env.step_simple(seed, 3)                      # agents with a memory, a handle whose tick is not 0
        before = env.counters(), env.episodes()
        games, out = pa.new_games(n), torch.full((n,), -1, dtype=torch.int32, device="cuda")
        assert env.deal(games, seed=SEED, out=out) is out
        got = env.get_state()
        assert got.tobytes() == want.tobytes(), np.flatnonzero([got[e].tobytes() != want[e].tobytes() for e in range(n)])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_words) and games.cpu().tolist() == [1] * n
        d = pa.decode_deal(out)
        assert d["dealt"].all() and not d["fallback"].any() and (d["bad"] <= 4).all()
        assert not env.policy_memory().any() and not env.status()["done"].any() and not env.status()["ubflags"].any()
        assert np.array_equal(env.counters(), before[0]) and np.array_equal(env.episodes(), before[1])
        # the dealt games play like the checker's under the CPU oracle, restarts on the dealt boards included; the handle's tick is
        # still the 3 it was
        env.step_simple(seed, 40)
        ref, mems = want.copy(), np.zeros((n, 4, 16), dtype=np.int32)
        oracle.run_simple(ref, want, mems, 40, seed, offset, 3, cap)
        assert env.get_state().tobytes() == ref.tobytes() and np.array_equal(env.policy_memory(), mems)
        # the second deal of an env is its board 1
        env.deal(games, seed=SEED, first=n - 2, out=out)
        assert env.get_state(n - 2, 2).tobytes() == Boards(env_offset=offset).many([n - 2, n - 1], [1, 1])[0].tobytes()
        assert games.cpu().tolist() == [1] * (n - 2) + [2, 2]


@pytest.mark.parametrize("which", ["range", "mask"])
def test_envs_that_are_not_dealt_keep_everything(hip_lib, boards, which):
    """a range that is no whole tile (first 3, count 22, of 37), and a random mask over the whole batch"""
    import torch
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    n, first, count, sentinel = 37, 3, 22, 0x5A5A5A5A
    if which == "range":
        dealt, kw = (np.arange(n) >= first) & (np.arange(n) < first + count), dict(first=first, count=count)
        in_range = dealt
    else:
        dealt, in_range = np.random.default_rng(4).random(n) < 0.5, np.ones(n, dtype=bool)
        assert dealt[:16].any() and not dealt[:16].all() and 5 < dealt.sum() < n - 5
        kw = dict(which=torch.from_numpy(dealt.astype(np.int32) * 7).cuda())
    start = pa.make_boards(n, seed=8)
    with BatchEnvironment(n, mode=MODE_ENV, max_steps=25) as env:
        env.make_game(start)
        env.step_simple(2, 30)                        # memories, finished envs, counters
        before = _everything(env)
        assert before["status_done"].any() and before["memory"].any()
        g0 = np.arange(n, dtype=np.int32) % 3
        games, out = torch.from_numpy(g0.copy()).cuda(), torch.full((n,), sentinel, dtype=torch.int32, device="cuda")
        env.deal(games, seed=SEED, out=out, **kw)
        after = _everything(env)
        want, want_words = boards.many(np.flatnonzero(dealt), g0[dealt])
        for k in before:
            if k in ("episodes", "counters"):
                assert np.array_equal(after[k], before[k]), k
            else:
                assert after[k][~dealt].tobytes() == before[k][~dealt].tobytes(), k
        assert after["state"][dealt].tobytes() == want.tobytes() and not after["memory"][dealt].any()
        assert not after["status_done"][dealt].any() and not after["status_ubflags"][dealt].any()
        words = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(words[dealt], want_words) and (words[in_range & ~dealt] == 0).all() and (words[~in_range] == sentinel).all()
        assert np.array_equal(games.cpu().numpy(), g0 + dealt)
        snap = _snapshots(env)
        assert snap[dealt].tobytes() == want.tobytes() and snap[~dealt].tobytes() == start[~dealt].tobytes()


def test_next_changes_the_snapshot_only(hip_lib, boards):
    import torch
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    n = 37
    with BatchEnvironment(n, mode=MODE_ENV, max_steps=25) as env:
        env.make_game(pa.make_boards(n, seed=8))
        env.step_simple(2, 30)
        before = _everything(env)
        g0 = (np.arange(n, dtype=np.int32) * 5) % 4
        games, out = torch.from_numpy(g0.copy()).cuda(), torch.zeros((n,), dtype=torch.int32, device="cuda")
        env.deal(games, seed=SEED, mode="next", out=out)
        after = _everything(env)
        assert all(np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes() for k in before)
        want, want_words = boards.many(range(n), g0)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want_words) and np.array_equal(games.cpu().numpy(), g0 + 1)
        assert _snapshots(env).tobytes() == want.tobytes()


def test_start_restarted_deals_the_envs_the_tick_restarted_and_keeps_their_last_episode(hip_lib, boards):
    """RESET_AT_END: START with which = "restarted" deals exactly the envs the last tick restarted — record, snapshot, fresh memory, status
    clear — and leaves their finished episode's results and terminal record, and every other env, as they were; then "done" on a handle
    whose finished envs stay finished."""
    import torch
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END
    n, sentinel = 37, 0x5A5A5A5A
    start = pa.make_boards(n, seed=8)
    for reset, which in ((RESET_AT_END, "restarted"), (0, "done")):
        at_end = reset == RESET_AT_END
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=reset, max_steps=25) as env:
            env.make_game(start)
            env.step_simple(2, 12)
            env.restore(np.arange(n) % 3 == 0)   # out of lockstep: a third of the envs starts again here, so tick 25 ends the games of a part only
            env.step_simple(2, 13)
            before = _everything(env, at_end)
            dealt = (before["last_finished"] != 0) if at_end else (before["status_done"] != 0)
            assert dealt.any() and not dealt.all() and dealt[:16].any() and not dealt[:16].all(), dealt
            if at_end:
                assert before["terminal"][dealt]["timeStep"].all() and (before["last_length"][dealt] > 0).all()
            g0 = np.arange(n, dtype=np.int32) % 3
            games, out = torch.from_numpy(g0.copy()).cuda(), torch.full((n,), sentinel, dtype=torch.int32, device="cuda")
            env.deal(games, seed=SEED, which=which, out=out)
            after = _everything(env, at_end)
            want, want_words = boards.many(np.flatnonzero(dealt), g0[dealt])
            for k in before:
                if k in ("episodes", "counters", "terminal") or (k.startswith("last_") and k != "last_finished"):
                    assert np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes(), k   # dealt or not
                else:
                    assert after[k][~dealt].tobytes() == before[k][~dealt].tobytes(), k
            assert after["state"][dealt].tobytes() == want.tobytes() and not after["memory"][dealt].any()
            assert not after["status_done"][dealt].any() and not after["status_ubflags"][dealt].any()
            if at_end:
                assert not after["last_finished"][dealt].any()   # the "restarted" bit is status, and START clears the status
            words = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(words[dealt], want_words) and (words[~dealt] == 0).all()
            assert np.array_equal(games.cpu().numpy(), g0 + dealt)
            snap = _snapshots(env)
            assert snap[dealt].tobytes() == want.tobytes() and snap[~dealt].tobytes() == start[~dealt].tobytes()


def _closed_loop(env, model, boards, which, ticks, rng):
    """`ticks` ticks of step_device with random moves, deal(NEXT, which) behind each; the model's snapshots refilled from the checker"""
    import torch
    import pomcpp_amd as pa
    n = env.n
    games, g = pa.new_games(n), np.zeros(n, dtype=np.int64)

    def model_deal(envs, start=False):
        for e in envs:
            model.snapshot[e] = boards(e, g[e])[0]
            if start:
                model.states[e] = model.snapshot[e]
            g[e] += 1
    env.deal(games, seed=SEED)
    model_deal(range(n), start=True)
    env.deal(games, seed=SEED, mode="next")
    model_deal(range(n))
    restarts = np.zeros(n, dtype=np.int64)
    for t in range(ticks):
        moves = rng.integers(0, 6, size=(n, 4)).astype(np.int32)
        env.step_device(torch.from_numpy(moves).cuda())
        env.deal(games, seed=SEED, mode="next", which=which)
        log = model.tick(0, n, moves)
        todo = log["restarted"] if which == "restarted" else np.flatnonzero(model.done).tolist()
        if which == "done":
            restarts[log["restarted"]] += 1
        else:
            restarts[todo] += 1
        model_deal(todo)
        model.same_as(env, f"tick {t}")   # every tick: a record that goes wrong shortly before a restart is put right by the restart
        assert np.array_equal(games.cpu().numpy(), g), t
    return restarts, g


@pytest.mark.parametrize("reset,which", [(2, "restarted"), (1, "done")])
def test_closed_loop_every_game_on_a_new_board(hip_lib, oracle, boards, reset, which):
    """n = 37, max_steps 25 so that games end often, 120 ticks.  Everything the API can read of the handle — states, status, episodes,
    counters, terminal records and last results — and the game counters are compared with the model after every tick."""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    n, cap = 37, 25
    start = pa.make_boards(n, seed=1)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=reset, max_steps=cap) as env:
        env.make_game(start)
        model = RangeModel(oracle, start, max_steps=cap, auto_reset=reset)
        restarts, g = _closed_loop(env, model, boards, which, 120, np.random.default_rng(6))
        assert (restarts >= 2).all(), restarts
        # every restart landed on the next board of its env: no board was replayed, none skipped
        assert np.array_equal(g, 2 + restarts + (model.done != 0 if which == "done" else 0))


def test_refusals_that_need_a_handle(hip_lib, boards):
    import torch
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, _BoardLayout, _DealSpec
    lib, n = hip_lib, 20
    games, out = pa.new_games(n), torch.full((n,), 9, dtype=torch.int32, device="cuda")

    def spec(**kw):
        f = dict(mode=0, which=0, reserved_=0, first=0, count=n, seed=1, layout=_BoardLayout(*DO.STANDARD), reserved2_=0, games_dev=games.data_ptr(),
                 which_dev=None, result_dev=out.data_ptr(), stream=None)
        f.update(kw)
        return _DealSpec(C.sizeof(_DealSpec), *[f[name] for name, _ in _DealSpec._fields_[1:]])

    def refused(env, named, **kw):
        before = env.get_state()
        assert lib.pom_batch_destroy(None) == 1       # another call's text stands in pom_last_error
        rc, text = lib.pom_batch_deal(env._h, C.byref(spec(**kw))), lib.pom_last_error().decode()
        assert rc == 1 and text.startswith("pom_batch_deal: ") and named in text, (kw, rc, text)
        assert env.get_state().tobytes() == before.tobytes() and games.cpu().tolist() == [0] * n and out.cpu().tolist() == [9] * n
    with BatchEnvironment(n, mode=MODE_ENV, max_steps=25) as env:
        env.make_game(pa.make_boards(n, seed=8))
        for kw in (dict(first=-1), dict(first=15, count=11), dict(first=n + 1, count=0), dict(count=n + 1)):
            refused(env, "outside the batch", **kw)
        refused(env, "POM_RESET_AT_END", which=2)
        refused(env, "num_rigid", layout=_BoardLayout(35, 36, 20, 4, 0))
        assert lib.pom_batch_deal(env._h, C.byref(spec(count=0, first=n, games_dev=None))) == 0   # nothing to do is no error
        with pytest.raises(pa.PomError, match="POM_RESET_AT_END"):
            env.deal(games, which="restarted")
    with BatchEnvironment(n, mode=MODE_ENV, lanes_per_env=1) as env:
        env.make_game(pa.make_boards(n, seed=8))
        refused(env, "quad launch shape")
