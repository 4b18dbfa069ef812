"""pom_batch_forecast on the GPU (include/pom_batch.h PomForecastSpec): flames and deaths K ticks ahead, bit-exact against the
compiled reference's answers (tests/golden/forecast.npz), the checker (tests/forecast_oracle.py: K x Oracle.step on a copy) and the
existing step and observation kernels; and the batch is left exactly as it was.  The states are played on the CPU and uploaded, so
what the forecast has to say is known before the GPU runs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests.forecast_oracle import forecast

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "forecast.npz")
KINDS = [("ffa", 57), ("stress", 23)]
SIZES = [5, 16, 67, 200]          # a short last tile, one whole tile, n no multiple of 4, several tiles
HORIZONS = [1, 4, 12, 32]


@functools.lru_cache(maxsize=None)
def _played(kind, n, ticks):
    from tests.oracle_lib import Oracle
    s = FC.played_states(Oracle(), kind, n, ticks)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _want(kind, n, ticks, horizon, with_moves):
    """the checker's three outputs, computed once and shared (nobody writes to them)"""
    from tests.oracle_lib import Oracle
    mv = FC.random_moves(n, 11 * n + horizon) if with_moves else None
    out = forecast(Oracle(), _played(kind, n, ticks), horizon, mv) + (mv,)
    for a in out[:3]:
        a.setflags(write=False)
    return out


def _env(states, **kw):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    kw.setdefault("mode", MODE_ENV)
    env = BatchEnvironment(len(states), **kw)
    env.make_game(states)
    return env


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _same(got, want, what):
    flame, agent, ub = want[:3]
    g = got["flame_tick"].cpu().numpy()
    bad = np.nonzero((g != flame).any(axis=(1, 2)))[0]
    assert bad.size == 0, f"{what}: flame_tick of {bad.size} envs differs, first env {bad[0]}, cells (y, x) {np.argwhere(g[bad[0]] != flame[bad[0]])[:8].tolist()}"
    assert np.array_equal(got["agent_tick"].cpu().numpy(), agent), what
    if "ubflags" in got:
        assert np.array_equal(got["ubflags"].cpu().numpy().view(np.uint32), ub), what


@pytest.mark.gpu
def test_fixture_replay(hip_lib):
    """the fixture's starts uploaded grouped by (horizon, idle / moves): both outputs as the compiled reference gave them"""
    g = np.load(GOLDEN)
    groups = sorted({(int(h), int(m)) for h, m in zip(g["horizon"], g["has_moves"])})
    assert len(groups) >= 8
    for horizon, has_moves in groups:
        ix = np.nonzero((g["horizon"] == horizon) & (g["has_moves"] == has_moves))[0]
        states = np.ascontiguousarray(g["start"][ix]).view(STATE_DTYPE).reshape(-1)
        with _env(states) as env:
            got = env.forecast(horizon, moves=_dev(g["moves"][ix]) if has_moves else None, ubflags=True)
            _same(got, (g["flame_tick"][ix], g["agent_tick"][ix], np.zeros(ix.size, dtype=np.uint32)), f"horizon {horizon} moves {has_moves}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_forecast_matches_the_checker(hip_lib, kind, ticks, n):
    """every horizon, idle and with random first-tick moves; the outputs inside larger buffers of sentinels whose other bytes stay
    untouched (a short last tile must be clipped at byte n * 121)"""
    import torch
    states = _played(kind, n, ticks)
    with _env(states) as env:
        before = env.get_state().tobytes()
        for horizon in HORIZONS:
            for with_moves in (False, True):
                want = _want(kind, n, ticks, horizon, with_moves)
                fbuf = torch.full((16 + n * 121 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
                abuf = torch.full((4 + n * 4 + 16,), -7, dtype=torch.int32, device="cuda")
                ubuf = torch.full((1 + n + 16,), -7, dtype=torch.int32, device="cuda")
                assert fbuf.data_ptr() % 16 == 0 and abuf.data_ptr() % 16 == 0
                out = {"flame_tick": fbuf[16:16 + n * 121].view(n, 11, 11), "agent_tick": abuf[4:4 + n * 4].view(n, 4), "ubflags": ubuf[1:1 + n]}
                got = env.forecast(horizon, moves=_dev(want[3]), out=out, ubflags=True)
                assert got["flame_tick"].data_ptr() == out["flame_tick"].data_ptr()
                _same(got, want, f"{kind} n {n} horizon {horizon} moves {with_moves}")
                assert (fbuf[:16] == 0xAB).all() and (fbuf[16 + n * 121:] == 0xAB).all()
                assert (abuf[:4] == -7).all() and (abuf[4 + n * 4:] == -7).all() and ubuf[0] == -7 and (ubuf[1 + n:] == -7).all()
        assert env.get_state().tobytes() == before
        only = env.forecast(4, agent_ticks=False)
        assert set(only) == {"flame_tick"} and np.array_equal(only["flame_tick"].cpu().numpy(), _want(kind, n, ticks, 4, False)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_second_witness_step_and_observe(hip_lib, kind, ticks):
    """the existing kernels as the yardstick: a RAW twin plays m_1, then IDLE, with the code planes exported after every tick; the
    first tick each cell shows flames (board code 4) and each agent turns up dead is the forecast"""
    import torch
    from pomcpp_amd.batch import MODE_RAW
    n, horizon = 200, 12
    states = _played(kind, n, ticks)
    mv = _dev(FC.random_moves(n, 5))
    idle = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    with _env(states) as env, _env(states, mode=MODE_RAW) as twin:
        got = env.forecast(horizon, moves=mv)
        flame = torch.zeros((n, 11, 11), dtype=torch.uint8, device="cuda")
        _, attrs, _ = twin.observe(dtype="codes")
        agent = torch.where(attrs[:, :, 2] == 0, -1, 0).to(torch.int32)
        for t in range(1, horizon + 1):
            twin.step_device(mv if t == 1 else idle)               # two launches, not the fused one: the plain step kernel ...
            codes, attrs, _ = twin.observe(dtype="codes")          # ... and the export kernel
            flame = torch.where((codes[:, 0] == 4) & (flame == 0), torch.full_like(flame, t), flame)
            agent = torch.where((agent == 0) & (attrs[:, :, 2] == 0), torch.full_like(agent, t), agent)
        assert (got["flame_tick"] == flame).all() and (got["agent_tick"] == agent).all()
        assert int((flame > 0).sum()) > n and int((agent > 0).sum()) > 0


def _everything(env):
    """all the API can read of a handle"""
    out = dict(state=env.get_state().tobytes(), terminal=env.get_terminal_state().tobytes(), counters=env.counters().tolist(),
               episodes=env.episodes().tolist(), memory=env.policy_memory().tobytes(), chain=env.chain_stats())
    out.update({"status_" + k: v.tolist() for k, v in env.status().items()})
    out.update({"last_" + k: v.tolist() for k, v in env.last_results().items()})
    return out


@pytest.mark.gpu
def test_forecast_leaves_no_trace(hip_lib):
    """an ENV-mode handle with end-of-tick resets and fresh boards, in the middle of SimpleAgent games: everything the API can read is
    the same before and after forecasts, and 20 more ticks equal a twin's that never forecast"""
    from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
    n, kw = 200, dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    with BatchEnvironment(n, **kw) as env, BatchEnvironment(n, **kw) as twin:
        for e in (env, twin):
            e.generate(9)
            e.step_simple(3, 40)
        before = _everything(env)
        assert _everything(twin) == before   # (both handles have now been read once: each settled its chained launches once)
        assert sum(before["last_finished"]) + sum(before["episodes"]) > 0 and before["counters"][0] == n * 40
        for horizon, mv in ((12, _dev(FC.random_moves(n, 1))), (32, None), (1, _dev(FC.random_moves(n, 2)))):
            got = env.forecast(horizon, moves=mv, ubflags=True)
            assert int((got["flame_tick"] > 0).sum()) > 0 or horizon == 1
            assert _everything(env) == before, horizon
        env.step_simple(3, 20)
        env.forecast(8)
        twin.step_simple(3, 20)
        assert _everything(env) == _everything(twin)


@pytest.mark.gpu
def test_forecast_after_chained_launches_settles(hip_lib, oracle):
    """20 chained ticks, then the forecast with nothing in between: it starts from the state a download returns"""
    from pomcpp_amd.batch import DIST_RANDOM, ISSUE_CHAIN, MODE_ENV
    n = 600
    with _env(_played("stress", n, 23), mode=MODE_ENV, auto_reset=True, max_steps=300, issue_mode=ISSUE_CHAIN) as env:
        assert env.issue_info()[0] == "chain"
        env.step_random(5, DIST_RANDOM, ticks=20)
        launches = env.chain_stats()["launches"]
        got = env.forecast(12, ubflags=True)
        assert launches == 20 and env.chain_stats()["launches"] == 20
        _same(got, forecast(oracle, env.get_state(), 12), "after 20 chained ticks")


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", [(16, 1), (32, 1), (64, 1)])
def test_handle_shapes_give_the_same_outputs(hip_lib, epw, lpe):
    """the forecast's own launch shape does not depend on the handle's: the device buffers are 16-env tiles whatever the shape"""
    n = 67
    want = _want("stress", n, 23, 12, True)
    with _env(_played("stress", n, 23), envs_per_wave=epw, lanes_per_env=lpe) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        _same(env.forecast(12, moves=_dev(want[3]), ubflags=True), want, f"epw {epw}")


@pytest.mark.gpu
def test_outputs_do_not_depend_on_the_wavefront_mates(hip_lib, oracle):
    """every actor of tests/tile_mates.py (deep chains, claim-map victims, bounce chains, queue limits) in each of the 16 columns of a
    tile of its own, the other 15 columns played stress boards: what the forecast says of it is the checker's solo answer, wherever
    it sits and whoever sits beside it — the tile stays in LDS for 16 ticks and the scratch rows are never re-initialised"""
    from tests import tile_mates as TM
    entries = TM.actors(oracle)
    A, horizon = len(entries), TM.TICKS
    start = np.concatenate([e.start for e in entries])
    first = np.stack([e.moves[0] for e in entries]).astype(np.int32)
    want = forecast(oracle, start, horizon, first)
    assert int((want[0] > 0).sum()) > 1000 and (want[2] != 0).any()   # they burn, and LOST_AGENT travels along
    mates = _played("stress", 240, 23)
    who = np.repeat(np.arange(A), 16)                    # tile k: actor k // 16 ...
    col = np.tile(np.arange(16), A)                      # ... in column k % 16
    n = A * 16 * 16
    states = mates[np.arange(n) % mates.size].copy()
    moves = FC.random_moves(n, 3)
    at = np.arange(A * 16) * 16 + col
    states[at], moves[at] = start[who], first[who]
    with _env(states) as env:
        got = env.forecast(horizon, moves=_dev(moves), ubflags=True)
        sel = _dev(at.astype(np.int64))
        picked = {k: v[sel] for k, v in got.items()}
        _same(picked, (want[0][who], want[1][who], want[2][who]), "actors among stress mates")


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header, with a message, and nothing written"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _ForecastSpec
    n = 32
    with _env(_played("ffa", 67, 57)[:n].copy()) as env:
        lib, h = env._lib, env._h
        fbuf = torch.full((n * 121 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
        ibuf = torch.full((n * 4 + 64,), -7, dtype=torch.int32, device="cuda")
        mv = torch.zeros((n * 4 + 16,), dtype=torch.int32, device="cuda")
        size, f, a, m = C.sizeof(_ForecastSpec), fbuf.data_ptr(), ibuf.data_ptr(), mv.data_ptr()
        zero = lambda: (C.c_int32 * 2)(0, 0)  # noqa: E731
        bad = {
            "struct_size": _ForecastSpec(size - 8, 4, zero(), None, f, None, None),
            "horizon 0": _ForecastSpec(size, 0, zero(), None, f, None, None),
            "horizon 33": _ForecastSpec(size, 33, zero(), None, f, None, None),
            "reserved 0": _ForecastSpec(size, 4, (C.c_int32 * 2)(1, 0), None, f, None, None),
            "reserved 1": _ForecastSpec(size, 4, (C.c_int32 * 2)(0, 1), None, f, None, None),
            "null flame_tick": _ForecastSpec(size, 4, zero(), m, None, a, a),
            "flame_tick + 8": _ForecastSpec(size, 4, zero(), None, f + 8, None, None),
            "agent_tick + 4": _ForecastSpec(size, 4, zero(), None, f, a + 4, None),
            "ubflags + 2": _ForecastSpec(size, 4, zero(), None, f, None, a + 2),
            "moves + 1": _ForecastSpec(size, 4, zero(), m + 1, f, None, None),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_forecast(h, C.byref(spec)))
            assert err.value.code == 1 and "pom_batch_forecast" in str(err.value), what
        good = _ForecastSpec(size, 4, zero(), None, f, None, None)
        for call in (lambda: lib.pom_batch_forecast(None, C.byref(good)), lambda: lib.pom_batch_forecast(h, None)):
            with pytest.raises(PomError) as err:
                _check(lib, call())
            assert err.value.code == 1 and str(err.value)
        env.sync()
        assert (fbuf == 0xAB).all() and (ibuf == -7).all()
        assert env.get_state().tobytes() == before
        for kw in (dict(horizon=0), dict(horizon=33), dict(horizon=4, moves=mv[:n * 4].view(n, 4).to(torch.int64)),
                   dict(horizon=4, out={"flame_tick": fbuf[:n * 121].view(n, 121)})):
            with pytest.raises(ValueError):
                env.forecast(**kw)
        # ubflags_dev and moves_dev need 4-byte alignment only: a forecast 4 bytes into both buffers runs
        _check(lib, lib.pom_batch_forecast(h, C.byref(_ForecastSpec(size, 4, zero(), m + 4, f, a, a + 16 * n + 4))))   # ints 129 .. 160 of 192
        env.sync()
        assert not (fbuf[:n * 121] == 0xAB).any()
