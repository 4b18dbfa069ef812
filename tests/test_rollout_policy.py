"""pom_batch_rollout_policy on the GPU (include/pom_batch.h PomRolloutPolicySpec): playouts in which the agents of a mask play
SimpleAgent, bit-exact against the compiled reference's playouts (tests/golden/rollout_policy.npz), the checker
(tests/rollout_policy_oracle.py: the loop over Oracle.simple_policy and Oracle.step), the existing step and policy kernels and the
existing rollout; and the batch is left exactly as it was.  The states are played on the CPU and uploaded, so what the rollout has
to say is known before the GPU runs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests import rollout_oracle as RO
from tests import rollout_policy_oracle as PO
from tests.rollout_gpu import POOL, _dev, _env, _everything, _played, _same, _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rollout_policy.npz")
SIZES = [5, 16, 67, 200]          # a short last tile, one whole tile, n no multiple of 4, several tiles
SAMPLES = [1, 3]
HORIZONS = [1, 8, 48]
MASKS = [0xF, 0xE, 0x5]
KINDS = [("ffa", 57, RO.DIST_RANDOM), ("stress", 23, RO.DIST_STRESS)]   # boards and the stream of the agents outside the mask
FIRST = 0x3                       # with `first`: agents 0 and 1 — a SimpleAgent and, under 0xE, the random one
SEED = 99


def _first_moves(horizon, n=POOL):
    return FC.random_moves(n, 13 + horizon)


@functools.lru_cache(maxsize=None)
def _want(kind, ticks, dist, horizon, simple, first, samples=max(SAMPLES), n=POOL, max_steps=0):
    """the checker's words for the whole pool and the most samples, computed once and shared (nobody writes to them): fewer samples
    and smaller batches are its leading rows and columns"""
    from tests.oracle_lib import Oracle
    w = PO.rollout(Oracle(), _played(kind, ticks)[:n], None, horizon, samples, SEED, dist, simple, first,
                   _first_moves(horizon)[:n] if first else None, max_steps)
    w.setflags(write=False)
    return w


@pytest.mark.gpu
def test_fixture_replay(hip_lib):
    """the words the compiled reference's Step and SimpleAgent gave"""
    g = np.load(GOLDEN)
    R, seed = int(g["samples"]), int(g["seed"])
    assert len(g["names"]) == 18
    for k in range(len(g["dist"])):
        states = np.ascontiguousarray(g["states"][k]).view(STATE_DTYPE).reshape(-1)
        with _env(states) as env:
            mv = _dev(g["moves"][k])
            for j in np.nonzero(g["kind"] == k)[0]:
                fm = int(g["first_mask"][j])
                got = env.rollout(int(g["horizon"][j]), R, seed, int(g["dist"][k]), moves=mv if fm else None,
                                  simple=int(g["simple_mask"][j]), first=fm)
                _same(got, g["result"][j], str(g["names"][j]))


@pytest.mark.gpu
@pytest.mark.parametrize("with_first", [False, True])
@pytest.mark.parametrize("simple", MASKS)
@pytest.mark.parametrize("kind,ticks,dist", KINDS)
def test_rollout_matches_the_checker(hip_lib, kind, ticks, dist, simple, with_first):
    """every size, sample count and horizon; the words inside a larger buffer of sentinels whose other dwords stay untouched (a short
    last tile writes its envs only); the state bytes are the same before and after"""
    import torch
    first = FIRST if with_first else 0
    seen = 0
    for n in SIZES:
        with _env(_played(kind, ticks)[:n].copy()) as env:
            before = env.get_state().tobytes()
            for horizon in HORIZONS:
                want = _want(kind, ticks, dist, horizon, simple, first)
                mv = _dev(_first_moves(horizon)[:n]) if with_first else None
                for R in SAMPLES:
                    buf = torch.full((4 + R * n + 16,), -7, dtype=torch.int32, device="cuda")
                    out = buf[4:4 + R * n].view(R, n)
                    assert out.data_ptr() % 16 == 0
                    got = env.rollout(horizon, R, SEED, dist, moves=mv, out=out, simple=simple, first=first)
                    assert got.data_ptr() == out.data_ptr()
                    _same(got, want[:R, :n], f"{kind} n {n} R {R} K {horizon} simple {simple:#x} first {first:#x}")
                    assert (buf[:4] == -7).all() and (buf[4 + R * n:] == -7).all()
                seen |= int(np.bitwise_or.reduce(want[:, :n], axis=None))
            assert env.get_state().tobytes() == before
    assert seen & RO.RO_DONE and seen >> RO.RO_WINNER_SHIFT & 7   # the cases are not one-sided


@pytest.mark.gpu
def test_carried_memory(hip_lib, oracle):
    """a handle in the middle of SimpleAgent games: the playouts go on from the agents' memory as policy_memory() reports it, or, with
    fresh_agents, from new agents — and the two differ"""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import DIST_RANDOM
    n, K, R = 96, 24, 2
    with _env(pa.make_boards(n, seed=21), max_steps=0) as env:
        env.step_simple(3, 40)
        states, mem = env.get_state(), env.policy_memory()
        st = env.status()
        start = ((st["done"] != 0) * RO.RO_DONE | (st["draw"] != 0) * RO.RO_DRAW | (st["winner"] + 1) << RO.RO_WINNER_SHIFT).astype(np.uint32)
        assert mem.any() and int((st["done"] != 0).sum()) < n
        carried = env.rollout(K, R, SEED, DIST_RANDOM, simple=0xF)
        fresh = env.rollout(K, R, SEED, DIST_RANDOM, simple=0xF, fresh_agents=True)
        _same(carried, PO.rollout(oracle, states, mem, K, R, SEED, DIST_RANDOM, 0xF, start=start), "carried memory")
        _same(fresh, PO.rollout(oracle, states, None, K, R, SEED, DIST_RANDOM, 0xF, start=start), "fresh agents")
        assert (_words(carried) != _words(fresh)).any()
        assert env.policy_memory().tobytes() == mem.tobytes() and env.get_state().tobytes() == states.tobytes()


def _fields_equal(w, st, end, start, max_steps):
    """the result words against a stepped twin's statuses and states, field by field"""
    assert np.array_equal(w & 0xF, ((end["agents"]["dead"] == 0) << np.arange(4)).sum(axis=1))
    assert np.array_equal([bin(v).count("1") for v in w & 0xF], st["alive"])
    assert np.array_equal((w & RO.RO_DONE) != 0, st["done"] != 0) and np.array_equal((w & RO.RO_DRAW) != 0, st["draw"] != 0)
    assert np.array_equal((w >> RO.RO_WINNER_SHIFT & 7).astype(np.int32) - 1, st["winner"])
    assert np.array_equal(w >> RO.RO_LENGTH_SHIFT, st["time_step"] - start["timeStep"])
    assert np.array_equal((w & RO.RO_TIMEOUT) != 0, (st["done"] != 0) & (st["time_step"] >= max_steps))
    assert np.array_equal((w & RO.RO_UB) != 0, st["ubflags"] != 0) and not (w & ~np.uint32(0xFFFF07FF)).any()


@pytest.mark.gpu
def test_second_witness_the_fused_policy_kernel(hip_lib):
    """the equivalence the header states for simple_mask 0xF with fresh agents: for every sample an ENV-mode twin (auto_reset 0, the
    same max_steps) is uploaded with the states and stepped with step_simple under seed_r; its statuses are the rollout's words"""
    from pomcpp_amd.batch import DIST_RANDOM
    n, R, K, max_steps = 200, 3, 24, 70
    states = _played("ffa", 57)
    with _env(states, max_steps=max_steps) as env, _env(states, max_steps=max_steps) as twin:
        start = env.get_state()
        got = _words(env.rollout(K, R, SEED, DIST_RANDOM, simple=0xF, fresh_agents=True))
        assert np.array_equal(got, _words(env.rollout(K, R, SEED, DIST_RANDOM, simple=range(4))))   # (this handle never ran the policy)
        ended = 0
        for r in range(R):
            twin.upload(start)
            twin.set_tick(0)
            twin.step_simple(RO.splitmix64(SEED + r), K)
            st = twin.status()
            _fields_equal(got[r], st, twin.get_state(), start, max_steps)
            ended += int((st["done"] != 0).sum())
        assert 0 < ended < R * n


@pytest.mark.gpu
def test_second_witness_mixed_mask(hip_lib):
    """simple_mask 0xA: per tick policy_simple(seed_r), the other agents' entries of the move buffer overwritten with the stream's
    moves, step_policy — the pattern pom_batch_moves_device documents"""
    import torch
    from pomcpp_amd.batch import DIST_RANDOM
    n, R, K, simple, max_steps = 67, 2, 8, 0xA, 62
    states = _played("ffa", 57)[:n].copy()
    with _env(states, max_steps=max_steps) as env, _env(states, max_steps=max_steps) as twin:
        start = env.get_state()
        got = _words(env.rollout(K, R, SEED, DIST_RANDOM, simple=simple, fresh_agents=True))
        mt = twin.moves_tensor()
        ended = 0
        for r in range(R):
            seed_r = RO.splitmix64(SEED + r)
            twin.upload(start)
            twin.set_tick(0)
            for t in range(K):
                twin.policy_simple(seed_r)
                stream = np.array([RO.rng_moves(seed_r, e, t, DIST_RANDOM) for e in range(n)], dtype=np.int32)
                with torch.cuda.stream(torch.cuda.ExternalStream(twin.stream_handle())):
                    for a in range(4):
                        if not simple >> a & 1:
                            mt[:, a] = _dev(stream[:, a])
                twin.step_policy()
            st = twin.status()
            _fields_equal(got[r], st, twin.get_state(), start, max_steps)
            ended += int((st["done"] != 0).sum())
        del mt
        assert 0 < ended < R * n


@pytest.mark.gpu
@pytest.mark.parametrize("with_moves", [False, True])
def test_without_simple_agents_it_is_the_existing_rollout(hip_lib, with_moves):
    """the header's equivalence between the two entry points, which launch two kernels: pom_batch_rollout_policy with an empty
    simple_mask (pom_rollout_policy_kernel<false>) and first_mask 0xF when it is given moves, 0 when not, gives pom_batch_rollout's
    (pom_rollout_kernel's) words bit for bit; and moves that no agent is named for are not read"""
    from pomcpp_amd.batch import DIST_STRESS
    n = 67
    mv = _dev(FC.random_moves(n, 5)) if with_moves else None
    with _env(_played("stress", 23)[:n].copy(), max_steps=40) as env:
        old = _words(env.rollout(48, 3, SEED, DIST_STRESS, moves=mv))
        assert np.array_equal(_words(env.rollout(48, 3, SEED, DIST_STRESS, moves=mv, simple=0)), old)   # first defaults to all four with moves
        assert np.array_equal(_words(env.rollout(48, 3, SEED, DIST_STRESS, moves=mv, simple=(), first=0xF if with_moves else 0)), old)
        if with_moves:   # moves given but no agent named: accepted and not read
            assert np.array_equal(_words(env.rollout(48, 3, SEED, DIST_STRESS, moves=mv, first=0)), _words(env.rollout(48, 3, SEED, DIST_STRESS)))


@pytest.mark.gpu
def test_prefix_properties(hip_lib):
    """sample r of an R = 8 call is sample r of an R = 3 call; and the first five envs of a 67-env batch give the words of a 5-env
    batch of the same five states — whoever shares their wavefront and its floods, whenever those finish, and whether the lanes beside
    them hold envs or lie past the batch's end"""
    from pomcpp_amd.batch import DIST_STRESS
    states = _played("stress", 23)
    with _env(states[:67].copy()) as big, _env(states[:5].copy()) as small:
        for simple in (0xF, 0x6):
            w8, w3 = (_words(big.rollout(48, R, SEED, DIST_STRESS, simple=simple)) for R in (8, 3))
            assert np.array_equal(w8[:3], w3)
            w5 = _words(small.rollout(48, 8, SEED, DIST_STRESS, simple=simple))
            assert np.array_equal(w8[:, :5], w5)
            lengths = w8 >> RO.RO_LENGTH_SHIFT
            assert len(set(lengths[:, :16].ravel().tolist())) > 4   # the mates of the first tile finish at many different ticks


@pytest.mark.gpu
def test_words_do_not_depend_on_the_wavefront_mates(hip_lib, oracle):
    """every actor of tests/tile_mates.py in each of the 16 columns of a tile of its own, the other 15 columns played stress boards, all
    four agents SimpleAgent: its words are the checker's solo answer, wherever it sits and whoever sits beside it — the wavefront's
    floods are dealt to all 16 quads, the tile stays in LDS for 16 ticks and the overlaid rows are never re-initialised"""
    from pomcpp_amd.batch import DIST_RANDOM
    from tests import tile_mates as TM
    entries = TM.actors(oracle)
    A, horizon, R = len(entries), TM.TICKS, 2
    start = np.concatenate([e.start for e in entries])
    mates = _played("stress", 23)
    who = np.repeat(np.arange(A), 16)                    # tile k: actor k // 16 ...
    col = np.tile(np.arange(16), A)                      # ... in column k % 16
    n = A * 16 * 16
    states = mates[np.arange(n) % mates.size].copy()
    at = np.arange(A * 16) * 16 + col
    states[at] = start[who]
    want = np.stack([PO.rollout(oracle, start[w:w + 1], None, horizon, R, SEED, DIST_RANDOM, 0xF, env_offset=int(e))[:, 0]
                     for w, e in zip(who, at)], axis=1)
    assert len(set((want >> RO.RO_LENGTH_SHIFT).ravel().tolist())) > 4
    with _env(states) as env:
        got = env.rollout(horizon, R, SEED, DIST_RANDOM, simple=0xF)
        _same(got[:, _dev(at.astype(np.int64))], want, "actors among stress mates")


@pytest.mark.gpu
def test_rollout_leaves_no_trace(hip_lib):
    """an ENV-mode handle with end-of-tick resets and fresh boards, in the middle of SimpleAgent games: everything the API can read,
    the agents' memory included, is the same before and after rollouts, and 20 more ticks equal a twin's that never rolled out"""
    from pomcpp_amd.batch import DIST_RANDOM, DIST_STRESS, MODE_ENV, RESET_AT_END, BatchEnvironment
    n, kw = 200, dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    with BatchEnvironment(n, **kw) as env, BatchEnvironment(n, **kw) as twin:
        for e in (env, twin):
            e.generate(9)
            e.step_simple(3, 40)
        before = _everything(env)
        assert _everything(twin) == before   # (both handles have now been read once: each settled its chained launches once)
        assert sum(before["last_finished"]) + sum(before["episodes"]) > 0 and before["counters"][0] == n * 40 and any(before["memory"])
        for horizon, R, dist, kwargs in ((12, 4, DIST_RANDOM, dict(simple=0xE, first=0x1, moves=_dev(FC.random_moves(n, 1)))),
                                         (48, 8, DIST_STRESS, dict(simple=0xF)), (1, 1, DIST_RANDOM, dict(simple=0x8, fresh_agents=True))):
            got = _words(env.rollout(horizon, R, 5, dist, **kwargs))
            assert 1 <= (got >> RO.RO_LENGTH_SHIFT).max() <= min(horizon, 25)
            assert _everything(env) == before, horizon
        env.step_simple(3, 20)
        env.rollout(8, 2, 5, simple=0xF)
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
        got = env.rollout(8, 2, SEED, DIST_RANDOM, simple=0xF)
        assert launches == 20 and env.chain_stats()["launches"] == 20
        st = env.status()
        word0 = (st["done"] != 0) * RO.RO_DONE | (st["draw"] != 0) * RO.RO_DRAW | (st["winner"] + 1) << RO.RO_WINNER_SHIFT
        word0 |= ((st["done"] != 0) & (st["time_step"] >= 300)) * RO.RO_TIMEOUT
        _same(got, PO.rollout(oracle, env.get_state(), None, 8, 2, SEED, DIST_RANDOM, 0xF, max_steps=300, start=word0.astype(np.uint32)),
              "after 20 chained ticks")


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe,raw", [(16, 1, False), (32, 1, False), (64, 1, False), (16, 4, True)])
def test_handle_shapes_give_the_same_words(hip_lib, epw, lpe, raw):
    """the rollout's own launch shape does not depend on the handle's; and a RAW handle's envs are rolled out with Environment::Step's
    bookkeeping like any other"""
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW
    n = 67
    want = _want("stress", 23, RO.DIST_STRESS, 48, 0xE, FIRST)
    with _env(_played("stress", 23)[:n].copy(), envs_per_wave=epw, lanes_per_env=lpe, mode=MODE_RAW if raw else MODE_ENV) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        got = env.rollout(48, 3, SEED, RO.DIST_STRESS, moves=_dev(_first_moves(48)[:n]), simple=0xE, first=FIRST)
        _same(got, want[:3, :n], f"epw {epw} raw {raw}")


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header, with a message, and nothing written"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _RolloutPolicySpec as Spec
    n = 32
    with _env(_played("ffa", 57)[:n].copy()) as env:
        lib, h = env._lib, env._h
        rbuf = torch.full((4 * n + 64,), -7, dtype=torch.int32, device="cuda")
        mv = torch.zeros((n * 4 + 16,), dtype=torch.int32, device="cuda")
        size, r, m = C.sizeof(Spec), rbuf.data_ptr(), mv.data_ptr()
        bad = {
            "struct_size": Spec(size - 8, 4, 4, 1, 7, None, r, 0xF, 0, 0, 0),
            "the old spec's size": Spec(48, 4, 4, 1, 7, None, r, 0xF, 0, 0, 0),
            "horizon 0": Spec(size, 0, 4, 1, 7, None, r, 0xF, 0, 0, 0),
            "horizon 1025": Spec(size, 1025, 4, 1, 7, None, r, 0xF, 0, 0, 0),
            "samples 0": Spec(size, 4, 0, 1, 7, None, r, 0xF, 0, 0, 0),
            "samples 257": Spec(size, 4, 257, 1, 7, None, r, 0xF, 0, 0, 0),
            "dist -1": Spec(size, 4, 4, -1, 7, None, r, 0xF, 0, 0, 0),
            "dist 3": Spec(size, 4, 4, 3, 7, None, r, 0xF, 0, 0, 0),
            "reserved": Spec(size, 4, 4, 1, 7, None, r, 0xF, 0, 0, 1),
            "null result": Spec(size, 4, 4, 1, 7, m, None, 0xF, 0, 0, 0),
            "result + 8": Spec(size, 4, 4, 1, 7, None, r + 8, 0xF, 0, 0, 0),
            "moves + 2": Spec(size, 4, 4, 1, 7, m + 2, r, 0xF, 0x1, 0, 0),
            "simple 16": Spec(size, 4, 4, 1, 7, None, r, 16, 0, 0, 0),
            "simple -1": Spec(size, 4, 4, 1, 7, None, r, -1, 0, 0, 0),
            "first 16": Spec(size, 4, 4, 1, 7, m, r, 0xF, 16, 0, 0),
            "first -1": Spec(size, 4, 4, 1, 7, m, r, 0xF, -1, 0, 0),
            "first without moves": Spec(size, 4, 4, 1, 7, None, r, 0xF, 0x1, 0, 0),
            "flags 2": Spec(size, 4, 4, 1, 7, None, r, 0xF, 0, 2, 0),
            "flags -1": Spec(size, 4, 4, 1, 7, None, r, 0xF, 0, -1, 0),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_rollout_policy(h, C.byref(spec)))
            assert err.value.code == 1 and "pom_batch_rollout_policy" in str(err.value), what
        good = Spec(size, 4, 4, 1, 7, None, r, 0xF, 0, 0, 0)
        for call in (lambda: lib.pom_batch_rollout_policy(None, C.byref(good)), lambda: lib.pom_batch_rollout_policy(h, None)):
            with pytest.raises(PomError) as err:
                _check(lib, call())
            assert err.value.code == 1 and "pom_batch_rollout_policy" in str(err.value)
        env.sync()
        assert (rbuf == -7).all()
        assert env.get_state().tobytes() == before
        for kw in (dict(horizon=0, samples=1, seed=1, simple=0xF), dict(horizon=4, samples=257, seed=1, simple=0xF),
                   dict(horizon=4, samples=1, seed=1, dist=3, simple=0xF), dict(horizon=4, samples=1, seed=1, simple=16),
                   dict(horizon=4, samples=1, seed=1, simple=[4]), dict(horizon=4, samples=1, seed=1, simple=0xF, first=-1),
                   dict(horizon=4, samples=1, seed=1, simple=0xF, first=[0]),          # first without moves
                   dict(horizon=4, samples=1, seed=1, first=0x1),
                   dict(horizon=4, samples=1, seed=1, simple=0xF, moves=mv[:n * 4].view(n, 4).to(torch.int64)),
                   dict(horizon=4, samples=2, seed=1, simple=0xF, out=rbuf[:n].view(1, n))):
            with pytest.raises(ValueError):
                env.rollout(**kw)
        # a non-null moves_dev with first_mask 0 is accepted and not read (here: not even aligned to an entry); the limits are accepted
        _check(lib, lib.pom_batch_rollout_policy(h, C.byref(Spec(size, 1024, 4, 2, 7, m + 4, r, 0xF, 0, 1, 0))))
        env.sync()
        assert not (rbuf[:4 * n] == -7).any() and (rbuf[4 * n:] == -7).all()
