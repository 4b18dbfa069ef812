"""pom_batch_rollout_jobs on the GPU (include/pom_batch.h PomRolloutJobsSpec): playouts for a device-side list of (source env, moves
of tick 1), bit-exact against the compiled reference's playouts indexed by source (tests/golden/rollout_policy.npz), the checker
(tests/rollout_jobs_oracle.py: the policy rollout's checker on the one source state, keyed by the source) and the existing call
indexed by source; "no job" entries give exactly 0; and the batch, the list and the moves are left exactly as they were.

The batch is 40 envs — two whole tiles and a short one of 8, n_pad > n — and the list 37 jobs — two whole groups of 16 and a short
one of 5, no multiple of 4 —: the smallest shapes with a tile boundary, a short tile, a short group and every kind of entry."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests import rollout_jobs_oracle as JO
from tests import rollout_oracle as RO
from tests.rollout_gpu import _dev, _env, _everything, _played, _same, _words

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "rollout_policy.npz")

N, N_PAD, M = 40, 64, 37   # (the buffers hold a multiple of 64 columns)
# group 0: sources of all three tiles (0..15, 16..31, the short 32..39), source 5 three times, a -1 among them;
# group 1: no job throughout; group 2 (short): source 5 again, and the entries n, n_pad - 1 and 2^40, which are >= n
SRC = np.array([0, 17, 33, 5, 5, 39, 16, 5, 31, 15, -1, 2, 38, 20, 9, 36] + [-1] * 16 + [5, N, N_PAD - 1, 1 << 40, 34], dtype=np.int64)
REAL = (SRC >= 0) & (SRC < N)
SAMPLES = [1, 3]
HORIZONS = [1, 8, 48]
MASKS = [(0xF, 0), (0xE, 0x3), (0x5, 0), (0, 0xF)]     # (simple_mask, first_mask)
KINDS = [("ffa", 57, RO.DIST_RANDOM), ("stress", 23, RO.DIST_STRESS)]
SEED = 99

assert SRC.size == M and REAL.sum() == 17 and (SRC == 5).sum() == 4


def _job_moves(horizon, m=M):
    """a row per JOB; the jobs of source 5 carry different rows"""
    mv = FC.random_moves(m, 29 + horizon)
    assert len({tuple(mv[j]) for j in np.nonzero(SRC == 5)[0]}) > 1 or m != M
    return mv


def _states(kind, ticks):
    return _played(kind, ticks)[:N].copy()


@functools.lru_cache(maxsize=None)
def _want(kind, ticks, dist, horizon, simple, first, max_steps=0, env_offset=0):
    """the checker's words for the hand-built list and the most samples, computed once (nobody writes to them)"""
    from tests.oracle_lib import Oracle
    w = JO.rollout_jobs(Oracle(), _played(kind, ticks)[:N], None, SRC, horizon, max(SAMPLES), SEED, dist, simple, first,
                        _job_moves(horizon) if first else None, max_steps, env_offset)
    w.setflags(write=False)
    return w


@pytest.mark.gpu
def test_fixture_replay(hip_lib):
    """the compiled reference's words, indexed by source: a list with repeats over the fixture's 24-env batches, all 18 groups"""
    g = np.load(GOLDEN)
    R, seed = int(g["samples"]), int(g["seed"])
    assert len(g["names"]) == 18
    for k in range(len(g["dist"])):
        states = np.ascontiguousarray(g["states"][k]).view(STATE_DTYPE).reshape(-1)
        src = JO.golden_jobs(states.size)
        with _env(states) as env:
            s, mv = _dev(src), _dev(g["moves"][k][src])
            for j in np.nonzero(g["kind"] == k)[0]:
                fm = int(g["first_mask"][j])
                got = env.rollout_jobs(s, int(g["horizon"][j]), R, seed, int(g["dist"][k]), moves=mv if fm else None,
                                       simple=int(g["simple_mask"][j]), first=fm)
                _same(got, g["result"][j][:, src], str(g["names"][j]))


@pytest.mark.gpu
@pytest.mark.parametrize("max_steps,env_offset", [(0, 0), (70, 1000)])
@pytest.mark.parametrize("simple,first", MASKS)
@pytest.mark.parametrize("kind,ticks,dist", KINDS)
def test_jobs_match_the_checker(hip_lib, kind, ticks, dist, simple, first, max_steps, env_offset):
    """the hand-built list with per-job moves, every horizon and sample count"""
    seen = 0
    with _env(_states(kind, ticks), max_steps=max_steps, env_offset=env_offset) as env:
        assert env.device_view()[1] == N_PAD
        src = _dev(SRC)
        for horizon in HORIZONS:
            want = _want(kind, ticks, dist, horizon, simple, first, max_steps, env_offset)
            mv = _dev(_job_moves(horizon)) if first else None
            for R in SAMPLES:
                got = env.rollout_jobs(src, horizon, R, SEED, dist, moves=mv, simple=simple, first=first)
                _same(got, want[:R], f"{kind} R {R} K {horizon} simple {simple:#x} first {first:#x} max_steps {max_steps}")
            assert not want[:, ~REAL].any() and want[:, REAL].all()
            seen |= int(np.bitwise_or.reduce(want, axis=None))
    if max_steps:
        assert seen & RO.RO_DONE


@pytest.mark.gpu
@pytest.mark.parametrize("simple", [0, 0xF])
def test_against_the_existing_call(hip_lib, simple):
    """an identity list is rollout(..., simple=, first=) word for word; any list is that result indexed by source when job j carries
    the source's row of moves; the words without a job are exactly 0; every word of out[R][m] is written and nothing behind it"""
    import torch
    K, R, first = 48, 3, 0x3
    full = FC.random_moves(N, 7)
    with _env(_states("stress", 23), max_steps=40) as env:
        old = _words(env.rollout(K, R, SEED, RO.DIST_STRESS, moves=_dev(full), simple=simple, first=first))
        ident = env.rollout_jobs(_dev(np.arange(N, dtype=np.int64)), K, R, SEED, RO.DIST_STRESS, moves=_dev(full), simple=simple, first=first)
        _same(ident, old, "identity list")
        mv = full[np.clip(SRC, 0, N - 1)]
        buf = torch.full((4 + R * M + 16,), -7, dtype=torch.int32, device="cuda")
        out = buf[4:4 + R * M].view(R, M)
        assert out.data_ptr() % 16 == 0
        got = env.rollout_jobs(_dev(SRC), K, R, SEED, RO.DIST_STRESS, moves=_dev(mv), out=out, simple=simple, first=first)
        assert got.data_ptr() == out.data_ptr()
        want = np.where(REAL, old[:, np.clip(SRC, 0, N - 1)], 0).astype(np.uint32)
        _same(got, want, "the list, indexed by source")
        assert (_words(got)[:, ~REAL] == 0).all() and not (got == -7).any()
        assert (buf[:4] == -7).all() and (buf[4 + R * M:] == -7).all()
        # without moves and masks: the random rollout's words
        plain = _words(env.rollout(K, R, SEED, RO.DIST_STRESS))
        _same(env.rollout_jobs(_dev(SRC), K, R, SEED, RO.DIST_STRESS), np.where(REAL, plain[:, np.clip(SRC, 0, N - 1)], 0).astype(np.uint32),
              "no moves, no masks")


@pytest.mark.gpu
@pytest.mark.parametrize("with_others", [False, True])
def test_move_table_is_six_rollout_calls(hip_lib, with_others):
    """... each with its own moves — the agent's column set to the move — and the same simple, stacked"""
    K, R, agent, simple = 8, 3, 1, 0xD
    others = FC.random_moves(N, 3)
    with _env(_states("ffa", 57)) as env:
        table = env.move_table(agent, K, R, SEED, RO.DIST_RANDOM, others=_dev(others) if with_others else None, simple=simple)
        assert tuple(table.shape) == (6, R, N)
        want = []
        for c in range(6):
            mv = others.copy()
            mv[:, agent] = c
            want.append(_words(env.rollout(K, R, SEED, RO.DIST_RANDOM, moves=_dev(mv), simple=simple, first=0xF if with_others else [agent])))
        want = np.stack(want)
        assert np.array_equal(_words(table), want)
        assert all((want[c] != want[0]).any() for c in (1, 2, 3, 4))   # the move matters (a bomb laid on tick 1 does not within 8 ticks)


@pytest.mark.gpu
def test_carried_memory(hip_lib, oracle):
    """a handle in the middle of SimpleAgent games: the jobs go on from their SOURCE's memory as policy_memory() reports it, or, with
    fresh_agents, from new agents — and the two differ"""
    import pomcpp_amd as pa
    K, R = 24, 2
    with _env(pa.make_boards(N, seed=21), max_steps=0) as env:
        env.step_simple(3, 40)
        states, mem = env.get_state(), env.policy_memory()
        st = env.status()
        start = ((st["done"] != 0) * RO.RO_DONE | (st["draw"] != 0) * RO.RO_DRAW | (st["winner"] + 1) << RO.RO_WINNER_SHIFT).astype(np.uint32)
        assert mem.any() and int((st["done"] != 0)[SRC[REAL]].sum()) < REAL.sum()
        src = _dev(SRC)
        carried = env.rollout_jobs(src, K, R, SEED, RO.DIST_RANDOM, simple=0xF)
        fresh = env.rollout_jobs(src, K, R, SEED, RO.DIST_RANDOM, simple=0xF, fresh_agents=True)
        _same(carried, JO.rollout_jobs(oracle, states, mem, SRC, K, R, SEED, RO.DIST_RANDOM, 0xF, start=start), "carried memory")
        _same(fresh, JO.rollout_jobs(oracle, states, None, SRC, K, R, SEED, RO.DIST_RANDOM, 0xF, start=start), "fresh agents")
        assert (_words(carried) != _words(fresh)).any()
        assert env.policy_memory().tobytes() == mem.tobytes() and env.get_state().tobytes() == states.tobytes()


@pytest.mark.gpu
def test_jobs_leave_no_trace(hip_lib):
    """an ENV-mode handle with end-of-tick resets and fresh boards, in the middle of SimpleAgent games: everything the API can read is
    the same before and after, and so are the list and the moves"""
    from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
    kw = dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    with BatchEnvironment(N, **kw) as env:
        env.generate(9)
        env.step_simple(3, 40)
        before = _everything(env)
        assert any(before["memory"]) and before["counters"][0] == N * 40
        src, mv = _dev(SRC), _dev(_job_moves(12))
        for horizon, R, dist, kwargs in ((12, 3, RO.DIST_RANDOM, dict(simple=0xE, first=0x1, moves=mv)), (48, 3, RO.DIST_STRESS, dict(simple=0xF)),
                                         (1, 1, RO.DIST_RANDOM, dict(fresh_agents=True))):
            got = _words(env.rollout_jobs(src, horizon, R, 5, dist, **kwargs))
            assert 1 <= (got >> RO.RO_LENGTH_SHIFT).max() <= min(horizon, 25)
            assert _everything(env) == before, horizon
        assert np.array_equal(src.cpu().numpy(), SRC) and np.array_equal(mv.cpu().numpy(), _job_moves(12))


@pytest.mark.gpu
def test_words_do_not_depend_on_the_group_mates(hip_lib):
    """a job's words are the same whoever fills the other 15 slots of its group — other sources, no job, nothing (the list's end) — and
    wherever in the list it stands"""
    K, R, simple, first = 48, 3, 0xE, 0x3
    mv = _job_moves(K)
    with _env(_states("stress", 23)) as env:
        base = _words(env.rollout_jobs(_dev(SRC), K, R, SEED, RO.DIST_STRESS, moves=_dev(mv), simple=simple, first=first))
        assert len(set((base[:, REAL] >> RO.RO_LENGTH_SHIFT).ravel().tolist())) > 4   # the mates finish at many different ticks
        perm = np.random.default_rng(3).permutation(M)
        got = _words(env.rollout_jobs(_dev(SRC[perm]), K, R, SEED, RO.DIST_STRESS, moves=_dev(mv[perm]), simple=simple, first=first))
        assert np.array_equal(got, base[:, perm])
        for j in (3, 5, 36):   # alone in its group: among 15 entries without a job, and as a list of one
            alone = np.full(16, -1, dtype=np.int64)
            alone[j % 16] = SRC[j]
            amv = np.zeros((16, 4), dtype=np.int32)
            amv[j % 16] = mv[j]
            got = _words(env.rollout_jobs(_dev(alone), K, R, SEED, RO.DIST_STRESS, moves=_dev(amv), simple=simple, first=first))
            assert np.array_equal(got[:, j % 16], base[:, j]) and not np.delete(got, j % 16, axis=1).any()
            one = _words(env.rollout_jobs(_dev(SRC[j:j + 1]), K, R, SEED, RO.DIST_STRESS, moves=_dev(mv[j:j + 1]), simple=simple, first=first))
            assert np.array_equal(one[:, 0], base[:, j])
        # among other sources: its group filled with envs that are not in the list
        crowd = np.array([1, 3, 4, 6, 7, 8, 10, 11, 12, 13, 14, 18, 19, 21, 22, 23], dtype=np.int64)
        crowd[9], cmv = SRC[5], FC.random_moves(16, 77)
        cmv[9] = mv[5]
        got = _words(env.rollout_jobs(_dev(crowd), K, R, SEED, RO.DIST_STRESS, moves=_dev(cmv), simple=simple, first=first))
        assert np.array_equal(got[:, 9], base[:, 5])


@pytest.mark.gpu
def test_jobs_after_chained_launches_settle(hip_lib, oracle):
    """20 chained ticks, then the jobs with nothing in between: they start from the state a download returns"""
    from pomcpp_amd.batch import ISSUE_CHAIN, MODE_ENV
    n = 600
    states = FC.played_states(oracle, "stress", n, 23)
    src = np.array([599, 0, 16, 599, -1, 300, 47, 123, n, 585, 31, 32, 200, 411, 16, 77, 5], dtype=np.int64)
    with _env(states, mode=MODE_ENV, auto_reset=True, max_steps=300, issue_mode=ISSUE_CHAIN) as env:
        assert env.issue_info()[0] == "chain"
        env.step_random(5, RO.DIST_RANDOM, ticks=20)
        launches = env.chain_stats()["launches"]
        got = env.rollout_jobs(_dev(src), 8, 2, SEED, RO.DIST_RANDOM, simple=0xF)
        assert launches == 20 and env.chain_stats()["launches"] == 20
        st = env.status()
        word0 = (st["done"] != 0) * RO.RO_DONE | (st["draw"] != 0) * RO.RO_DRAW | (st["winner"] + 1) << RO.RO_WINNER_SHIFT
        word0 |= ((st["done"] != 0) & (st["time_step"] >= 300)) * RO.RO_TIMEOUT
        _same(got, JO.rollout_jobs(oracle, env.get_state(), None, src, 8, 2, SEED, RO.DIST_RANDOM, 0xF, max_steps=300,
                                   start=word0.astype(np.uint32)), "after 20 chained ticks")


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe,raw", [(16, 1, False), (32, 1, False), (64, 1, False), (16, 4, True)])
def test_handle_shapes_give_the_same_words(hip_lib, epw, lpe, raw):
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW
    want = _want("stress", 23, RO.DIST_STRESS, 48, 0xE, 0x3)
    with _env(_states("stress", 23), envs_per_wave=epw, lanes_per_env=lpe, mode=MODE_RAW if raw else MODE_ENV) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        got = env.rollout_jobs(_dev(SRC), 48, 3, SEED, RO.DIST_STRESS, moves=_dev(_job_moves(48)), simple=0xE, first=0x3)
        _same(got, want[:3], f"epw {epw} raw {raw}")


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header on a live handle, with a message, and nothing written; an empty list is OK and writes nothing"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _RolloutJobsSpec as Spec
    with _env(_states("ffa", 57)) as env:
        lib, h = env._lib, env._h
        rbuf = torch.full((4 * M + 64,), -7, dtype=torch.int32, device="cuda")
        mv = torch.zeros((M * 4 + 16,), dtype=torch.int32, device="cuda")
        sr = _dev(np.concatenate([SRC, SRC[:3]]))
        size, r, m, s = C.sizeof(Spec), rbuf.data_ptr(), mv.data_ptr(), sr.data_ptr()
        assert r % 16 == 0 and s % 8 == 0
        bad = {
            "struct_size": Spec(size - 8, 4, 4, 1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "the policy spec's size": Spec(56, 4, 4, 1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "horizon 0": Spec(size, 0, 4, 1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "horizon 1025": Spec(size, 1025, 4, 1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "samples 0": Spec(size, 4, 0, 1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "samples 257": Spec(size, 4, 257, 1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "dist -1": Spec(size, 4, 4, -1, 7, M, s, None, r, 0xF, 0, 0, 0),
            "dist 3": Spec(size, 4, 4, 3, 7, M, s, None, r, 0xF, 0, 0, 0),
            "reserved": Spec(size, 4, 4, 1, 7, M, s, None, r, 0xF, 0, 0, 1),
            "jobs -1": Spec(size, 4, 4, 1, 7, -1, s, None, r, 0xF, 0, 0, 0),
            "null src": Spec(size, 4, 4, 1, 7, M, None, None, r, 0xF, 0, 0, 0),
            "src + 4": Spec(size, 4, 4, 1, 7, M, s + 4, None, r, 0xF, 0, 0, 0),
            "null result": Spec(size, 4, 4, 1, 7, M, s, m, None, 0xF, 0, 0, 0),
            "result + 8": Spec(size, 4, 4, 1, 7, M, s, None, r + 8, 0xF, 0, 0, 0),
            "moves + 2": Spec(size, 4, 4, 1, 7, M, s, m + 2, r, 0xF, 0x1, 0, 0),
            "simple 16": Spec(size, 4, 4, 1, 7, M, s, None, r, 16, 0, 0, 0),
            "simple -1": Spec(size, 4, 4, 1, 7, M, s, None, r, -1, 0, 0, 0),
            "first 16": Spec(size, 4, 4, 1, 7, M, s, m, r, 0xF, 16, 0, 0),
            "first -1": Spec(size, 4, 4, 1, 7, M, s, m, r, 0xF, -1, 0, 0),
            "first without moves": Spec(size, 4, 4, 1, 7, M, s, None, r, 0xF, 0x1, 0, 0),
            "flags 2": Spec(size, 4, 4, 1, 7, M, s, None, r, 0xF, 0, 2, 0),
            "flags -1": Spec(size, 4, 4, 1, 7, M, s, None, r, 0xF, 0, -1, 0),
            "more than one grid": Spec(size, 4, 256, 1, 7, 1 << 28, s, None, r, 0xF, 0, 0, 0),
            "a list beyond all grids": Spec(size, 4, 1, 1, 7, (1 << 63) - 1, s, None, r, 0xF, 0, 0, 0),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_rollout_jobs(h, C.byref(spec)))
            assert err.value.code == 1 and "pom_batch_rollout_jobs" in str(err.value), what
        good = Spec(size, 4, 4, 1, 7, M, s, None, r, 0xF, 0, 0, 0)
        for call in (lambda: lib.pom_batch_rollout_jobs(None, C.byref(good)), lambda: lib.pom_batch_rollout_jobs(h, None)):
            with pytest.raises(PomError) as err:
                _check(lib, call())
            assert err.value.code == 1 and "pom_batch_rollout_jobs" in str(err.value)
        # an empty list: OK, nothing written — with pointers and without
        _check(lib, lib.pom_batch_rollout_jobs(h, C.byref(Spec(size, 4, 4, 1, 7, 0, s, None, r, 0xF, 0, 0, 0))))
        _check(lib, lib.pom_batch_rollout_jobs(h, C.byref(Spec(size, 4, 4, 1, 7, 0, None, None, None, 0xF, 0, 0, 0))))
        empty = env.rollout_jobs(sr[:0], 4, 4, 1, simple=0xF)
        assert tuple(empty.shape) == (4, 0)
        env.sync()
        assert (rbuf == -7).all()
        assert env.get_state().tobytes() == before
        for kw in (dict(horizon=0, samples=1, seed=1), dict(horizon=4, samples=257, seed=1), dict(horizon=4, samples=1, seed=1, dist=3),
                   dict(horizon=4, samples=1, seed=1, simple=16), dict(horizon=4, samples=1, seed=1, first=[0]),   # first without moves
                   dict(horizon=4, samples=1, seed=1, moves=mv[:M * 4].view(M, 4).to(torch.int64)),
                   dict(horizon=4, samples=1, seed=1, moves=mv[:(M - 1) * 4].view(M - 1, 4)),                    # a row per JOB
                   dict(horizon=4, samples=2, seed=1, out=rbuf[:M].view(1, M))):
            with pytest.raises(ValueError):
                env.rollout_jobs(sr[:M], **kw)
        for src in (sr[:M].to(torch.int32), sr[:M].cpu(), sr[:36].view(2, 18), SRC):
            with pytest.raises(ValueError):
                env.rollout_jobs(src, 4, 1, 1)
        with pytest.raises(ValueError):
            env.move_table(4, 4, 1, 1)
        # a non-null moves_dev with first_mask 0 is accepted and not read; the limits are accepted
        _check(lib, lib.pom_batch_rollout_jobs(h, C.byref(Spec(size, 1024, 4, 2, 7, M, s, m + 4, r, 0xF, 0, 1, 0))))
        env.sync()
        assert not (rbuf[:4 * M] == -7).any() and (rbuf[4 * M:] == -7).all()
