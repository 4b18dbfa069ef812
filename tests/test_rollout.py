"""pom_batch_rollout on the GPU (include/pom_batch.h PomRolloutSpec): R random playouts of every env, bit-exact against the
compiled reference's playouts (tests/golden/rollout.npz), the checker (tests/rollout_oracle.py: the loop over Oracle.step) and the
existing step kernels; and the batch is left exactly as it was.  The states are played on the CPU and uploaded, so what the
rollout has to say is known before the GPU runs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests import rollout_oracle as RO
from tests.rollout_gpu import POOL, _dev, _env, _everything, _played, _same, _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout.npz")
SIZES = [5, 16, 67, 200]          # a short last tile, one whole tile, n no multiple of 4, several tiles
SAMPLES = [1, 3, 8]
HORIZONS = [1, 8, 48]
# boards x move stream: every distribution, and the stress boards under POM_DIST_RANDOM, where a tick raises POM_UB_NULL_BOMB
COMBOS = [("ffa", 57, RO.DIST_HARMLESS), ("ffa", 57, RO.DIST_RANDOM), ("stress", 23, RO.DIST_STRESS), ("stress", 23, RO.DIST_RANDOM)]
SEED = 99


def _first_moves(with_moves, horizon, n=POOL):
    return FC.random_moves(n, 13 + horizon) if with_moves else None


@functools.lru_cache(maxsize=None)
def _want(kind, ticks, dist, horizon, with_moves, max_steps=0):
    """the checker's words for the whole pool and the most samples, computed once and shared (nobody writes to them): fewer samples
    and smaller batches are its leading rows and columns"""
    from tests.oracle_lib import Oracle
    w = RO.rollout(Oracle(), _played(kind, ticks), horizon, max(SAMPLES), SEED, dist, _first_moves(with_moves, horizon), max_steps)
    w.setflags(write=False)
    return w


@pytest.mark.gpu
def test_fixture_replay(hip_lib):
    """the words the compiled reference gave: the played groups, and the hand-made entries brought to their S_0 by the step kernel"""
    from pomcpp_amd.batch import DIST_RANDOM
    g = np.load(GOLDEN)
    R, seed = int(g["samples"]), int(g["seed"])
    assert len(g["names"]) == 12
    for k in range(len(g["dist"])):
        states = np.ascontiguousarray(g["states"][k]).view(STATE_DTYPE).reshape(-1)
        with _env(states) as env:
            for j in np.nonzero(g["kind"] == k)[0]:
                got = env.rollout(int(g["horizon"][j]), R, seed, int(g["dist"][k]), moves=_dev(g["moves"][k]) if g["has_moves"][j] else None)
                _same(got, g["result"][j], str(g["names"][j]))
    for j, name in enumerate(g["hand_names"]):
        pre = np.ascontiguousarray(g["hand_pre"][j]).view(STATE_DTYPE).reshape(-1)
        with _env(pre, max_steps=int(g["hand_max_steps"][j])) as env:
            for _ in range(int(g["hand_pre_ticks"][j])):
                env.step(np.zeros((1, 4), dtype=np.int32))
            assert env.get_state().tobytes() == g["hand_start"][j].tobytes(), name
            got = env.rollout(int(g["hand_horizon"][j]), R, seed, DIST_RANDOM)
            _same(got, g["hand_result"][j][:, None], str(name))


@pytest.mark.gpu
@pytest.mark.parametrize("with_moves", [False, True])
@pytest.mark.parametrize("kind,ticks,dist", COMBOS)
def test_rollout_matches_the_checker(hip_lib, kind, ticks, dist, with_moves):
    """every size, sample count and horizon; the words inside a larger buffer of sentinels whose other dwords stay untouched (a short
    last tile writes its envs only); the state bytes are the same before and after"""
    import torch
    seen = 0
    for n in SIZES:
        with _env(_played(kind, ticks)[:n].copy()) as env:
            before = env.get_state().tobytes()
            for horizon in HORIZONS:
                want = _want(kind, ticks, dist, horizon, with_moves)
                mv = _first_moves(with_moves, horizon)
                mv = None if mv is None else _dev(mv[:n])
                for R in SAMPLES:
                    buf = torch.full((4 + R * n + 16,), -7, dtype=torch.int32, device="cuda")
                    out = buf[4:4 + R * n].view(R, n)
                    assert out.data_ptr() % 16 == 0
                    got = env.rollout(horizon, R, SEED, dist, moves=mv, out=out)
                    assert got.data_ptr() == out.data_ptr()
                    _same(got, want[:R, :n], f"{kind} dist {dist} n {n} R {R} K {horizon} moves {with_moves}")
                    assert (buf[:4] == -7).all() and (buf[4 + R * n:] == -7).all()
                seen |= int(np.bitwise_or.reduce(want[:, :n], axis=None))
            assert env.get_state().tobytes() == before
    # the cases are not one-sided: winners, finished games, and bit 7 where the issue says a flag is raised
    assert seen & RO.RO_DONE and seen >> RO.RO_WINNER_SHIFT & 7
    assert seen & RO.RO_UB or (kind, dist) != ("stress", RO.DIST_RANDOM)


@pytest.mark.gpu
@pytest.mark.parametrize("with_moves", [False, True])
def test_second_witness_the_step_kernels(hip_lib, with_moves):
    """the equivalence the header states: for every sample an ENV-mode twin (auto_reset 0, the same max_steps) is uploaded with the
    downloaded states and stepped under seed_r; its statuses are the rollout's words"""
    from pomcpp_amd.batch import DIST_RANDOM
    n, R, K, max_steps = 200, 3, 24, 70
    states = _played("ffa", 57)
    mv = _dev(FC.random_moves(n, 5)) if with_moves else None
    with _env(states, max_steps=max_steps) as env, _env(states, max_steps=max_steps) as twin:
        start = env.get_state()
        got = _words(env.rollout(K, R, SEED, DIST_RANDOM, moves=mv))
        ended = 0
        for r in range(R):
            seed_r = RO.splitmix64(SEED + r)
            twin.upload(start)
            if with_moves:
                twin.step_device(mv)
                twin.set_tick(1)
                twin.step_random(seed_r, DIST_RANDOM, K - 1, 1)
            else:
                twin.set_tick(0)
                twin.step_random(seed_r, DIST_RANDOM, K, 1)
            st, end = twin.status(), twin.get_state()
            w = got[r]
            assert np.array_equal(w & 0xF, ((end["agents"]["dead"] == 0) << np.arange(4)).sum(axis=1))
            assert np.array_equal([bin(v).count("1") for v in w & 0xF], st["alive"])
            assert np.array_equal((w & RO.RO_DONE) != 0, st["done"] != 0) and np.array_equal((w & RO.RO_DRAW) != 0, st["draw"] != 0)
            assert np.array_equal((w >> RO.RO_WINNER_SHIFT & 7).astype(np.int32) - 1, st["winner"])
            assert np.array_equal(w >> RO.RO_LENGTH_SHIFT, st["time_step"] - start["timeStep"])
            assert np.array_equal((w & RO.RO_TIMEOUT) != 0, (st["done"] != 0) & (st["time_step"] >= max_steps))
            assert np.array_equal((w & RO.RO_UB) != 0, st["ubflags"] != 0) and not (w & ~np.uint32(0xFFFF07FF)).any()
            ended += int((st["done"] != 0).sum())
        assert 0 < ended < R * n


@pytest.mark.gpu
def test_prefix_properties(hip_lib):
    """sample r of an R = 8 call is sample r of an R = 3 call; and the first five envs of a 67-env batch give the words of a 5-env
    batch of the same five states — whoever shares their wavefront, whenever those finish, and whether the lanes beside them hold
    envs or lie past the batch's end"""
    from pomcpp_amd.batch import DIST_STRESS
    states = _played("stress", 23)
    with _env(states[:67].copy()) as big, _env(states[:5].copy()) as small:
        w8, w3 = _words(big.rollout(48, 8, SEED, DIST_STRESS)), _words(big.rollout(48, 3, SEED, DIST_STRESS))
        assert np.array_equal(w8[:3], w3)
        w5 = _words(small.rollout(48, 8, SEED, DIST_STRESS))
        assert np.array_equal(w8[:, :5], w5)
        lengths = w8 >> RO.RO_LENGTH_SHIFT
        assert len(set(lengths[:, :16].ravel().tolist())) > 4   # the mates of the first tile finish at many different ticks


@pytest.mark.gpu
def test_words_do_not_depend_on_the_wavefront_mates(hip_lib, oracle):
    """every actor of tests/tile_mates.py (deep chains, claim-map victims, bounce chains, queue limits) in each of the 16 columns of a
    tile of its own, the other 15 columns played stress boards: its words are the checker's solo answer, wherever it sits and whoever
    sits beside it — the tile stays in LDS for 16 ticks and the scratch rows are never re-initialised"""
    from pomcpp_amd.batch import DIST_RANDOM
    from tests import tile_mates as TM
    entries = TM.actors(oracle)
    A, horizon, R = len(entries), TM.TICKS, 2
    start = np.concatenate([e.start for e in entries])
    first = np.stack([e.moves[0] for e in entries]).astype(np.int32)
    mates = _played("stress", 23)
    who = np.repeat(np.arange(A), 16)                    # tile k: actor k // 16 ...
    col = np.tile(np.arange(16), A)                      # ... in column k % 16
    n = A * 16 * 16
    states = mates[np.arange(n) % mates.size].copy()
    moves = FC.random_moves(n, 3)
    at = np.arange(A * 16) * 16 + col
    states[at], moves[at] = start[who], first[who]
    want = np.stack([RO.rollout(oracle, start[w:w + 1], horizon, R, SEED, DIST_RANDOM, first[w:w + 1], env_offset=int(e))[:, 0]
                     for w, e in zip(who, at)], axis=1)
    assert (want & RO.RO_UB).any() and len(set((want >> RO.RO_LENGTH_SHIFT).ravel().tolist())) > 4
    with _env(states) as env:
        got = env.rollout(horizon, R, SEED, DIST_RANDOM, moves=_dev(moves))
        _same(got[:, _dev(at.astype(np.int64))], want, "actors among stress mates")


@pytest.mark.gpu
def test_rollout_leaves_no_trace(hip_lib):
    """an ENV-mode handle with end-of-tick resets and fresh boards, in the middle of SimpleAgent games: everything the API can read is
    the same before and after rollouts, and 20 more ticks equal a twin's that never rolled out"""
    from pomcpp_amd.batch import DIST_RANDOM, DIST_STRESS, MODE_ENV, RESET_AT_END, BatchEnvironment
    n, kw = 200, dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    with BatchEnvironment(n, **kw) as env, BatchEnvironment(n, **kw) as twin:
        for e in (env, twin):
            e.generate(9)
            e.step_simple(3, 40)
        before = _everything(env)
        assert _everything(twin) == before   # (both handles have now been read once: each settled its chained launches once)
        assert sum(before["last_finished"]) + sum(before["episodes"]) > 0 and before["counters"][0] == n * 40
        for horizon, R, dist, mv in ((12, 4, DIST_RANDOM, _dev(FC.random_moves(n, 1))), (48, 8, DIST_STRESS, None), (1, 1, DIST_RANDOM, None)):
            got = _words(env.rollout(horizon, R, 5, dist, moves=mv))
            assert 1 <= (got >> RO.RO_LENGTH_SHIFT).max() <= min(horizon, 25)
            assert _everything(env) == before, horizon
        env.step_simple(3, 20)
        env.rollout(8, 2, 5)
        twin.step_simple(3, 20)
        assert _everything(env) == _everything(twin)


@pytest.mark.gpu
def test_rollout_after_chained_launches_settles(hip_lib, oracle):
    """20 chained ticks, then the rollout with nothing in between: it starts from the state a download returns"""
    from pomcpp_amd.batch import DIST_RANDOM, ISSUE_CHAIN, MODE_ENV
    n = 600
    states = FC.played_states(oracle, "stress", n, 23)
    with _env(states, mode=MODE_ENV, auto_reset=True, max_steps=300, issue_mode=ISSUE_CHAIN) as env:
        assert env.issue_info()[0] == "chain"
        env.step_random(5, DIST_RANDOM, ticks=20)
        launches = env.chain_stats()["launches"]
        got = env.rollout(8, 2, SEED, DIST_RANDOM)
        assert launches == 20 and env.chain_stats()["launches"] == 20
        st = env.status()
        word0 = (st["done"] != 0) * RO.RO_DONE | (st["draw"] != 0) * RO.RO_DRAW | (st["winner"] + 1) << RO.RO_WINNER_SHIFT
        word0 |= ((st["done"] != 0) & (st["time_step"] >= 300)) * RO.RO_TIMEOUT
        _same(got, RO.rollout(oracle, env.get_state(), 8, 2, SEED, DIST_RANDOM, max_steps=300, start=word0.astype(np.uint32)), "after 20 chained ticks")


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe,raw", [(16, 1, False), (32, 1, False), (64, 1, False), (16, 4, True)])
def test_handle_shapes_give_the_same_words(hip_lib, epw, lpe, raw):
    """the rollout's own launch shape does not depend on the handle's: the device buffers are 16-env tiles whatever the shape; and a
    RAW handle's envs are rolled out with Environment::Step's bookkeeping like any other"""
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW
    n = 67
    want = _want("stress", 23, RO.DIST_STRESS, 48, True)
    with _env(_played("stress", 23)[:n].copy(), envs_per_wave=epw, lanes_per_env=lpe, mode=MODE_RAW if raw else MODE_ENV) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        _same(env.rollout(48, 3, SEED, RO.DIST_STRESS, moves=_dev(_first_moves(True, 48)[:n])), want[:3, :n], f"epw {epw} raw {raw}")


@pytest.mark.gpu
def test_max_steps_of_the_handle_times_games_out(hip_lib):
    """max_steps 12 on boards whose games are 1 .. 57 ticks old: a game that lives long enough times out in the tick that brings
    timeStep to 12 — in tick 1 if it is there already (an uploaded record is not finished: the rule is looked at after a tick)"""
    K, max_steps = 8, 12
    states = _played("ffa", 57)
    want = _want("ffa", 57, RO.DIST_RANDOM, K, False, max_steps)
    timed = (want & RO.RO_TIMEOUT) != 0
    assert timed.sum() > want.size // 4 and (want & RO.RO_DONE == 0).sum() > 0
    age = states["timeStep"][np.nonzero(timed)[1]]
    assert np.array_equal((want >> RO.RO_LENGTH_SHIFT)[timed], np.maximum(max_steps - age, 1)) and len(set(age.tolist())) > 12
    with _env(states, max_steps=max_steps) as env:
        _same(env.rollout(K, max(SAMPLES), SEED, RO.DIST_RANDOM), want, f"max_steps {max_steps}")


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header, with a message, and nothing written"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _RolloutSpec
    n = 32
    with _env(_played("ffa", 57)[:n].copy()) as env:
        lib, h = env._lib, env._h
        rbuf = torch.full((4 * n + 64,), -7, dtype=torch.int32, device="cuda")
        mv = torch.zeros((n * 4 + 16,), dtype=torch.int32, device="cuda")
        size, r, m = C.sizeof(_RolloutSpec), rbuf.data_ptr(), mv.data_ptr()
        bad = {
            "struct_size": _RolloutSpec(size - 8, 4, 4, 1, 7, None, r, 0),
            "horizon 0": _RolloutSpec(size, 0, 4, 1, 7, None, r, 0),
            "horizon 1025": _RolloutSpec(size, 1025, 4, 1, 7, None, r, 0),
            "samples 0": _RolloutSpec(size, 4, 0, 1, 7, None, r, 0),
            "samples 257": _RolloutSpec(size, 4, 257, 1, 7, None, r, 0),
            "dist -1": _RolloutSpec(size, 4, 4, -1, 7, None, r, 0),
            "dist 3": _RolloutSpec(size, 4, 4, 3, 7, None, r, 0),
            "reserved": _RolloutSpec(size, 4, 4, 1, 7, None, r, 1),
            "null result": _RolloutSpec(size, 4, 4, 1, 7, m, None, 0),
            "result + 8": _RolloutSpec(size, 4, 4, 1, 7, None, r + 8, 0),
            "moves + 2": _RolloutSpec(size, 4, 4, 1, 7, m + 2, r, 0),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_rollout(h, C.byref(spec)))
            assert err.value.code == 1 and "pom_batch_rollout" in str(err.value), what
        good = _RolloutSpec(size, 4, 4, 1, 7, None, r, 0)
        for call in (lambda: lib.pom_batch_rollout(None, C.byref(good)), lambda: lib.pom_batch_rollout(h, None)):
            with pytest.raises(PomError) as err:
                _check(lib, call())
            assert err.value.code == 1 and "pom_batch_rollout" in str(err.value)
        env.sync()
        assert (rbuf == -7).all()
        assert env.get_state().tobytes() == before
        for kw in (dict(horizon=0, samples=1, seed=1), dict(horizon=1025, samples=1, seed=1), dict(horizon=4, samples=0, seed=1),
                   dict(horizon=4, samples=257, seed=1), dict(horizon=4, samples=1, seed=1, dist=3),
                   dict(horizon=4, samples=1, seed=1, moves=mv[:n * 4].view(n, 4).to(torch.int64)),
                   dict(horizon=4, samples=2, seed=1, out=rbuf[:n].view(1, n))):
            with pytest.raises(ValueError):
                env.rollout(**kw)
        # moves_dev needs 4-byte alignment only: a rollout 4 bytes into the move buffer runs, and the limits themselves are accepted
        _check(lib, lib.pom_batch_rollout(h, C.byref(_RolloutSpec(size, 1024, 4, 2, 7, m + 4, r, 0))))
        env.sync()
        assert not (rbuf[:4 * n] == -7).any() and (rbuf[4 * n:] == -7).all()
