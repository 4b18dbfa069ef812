"""pom_batch_move_safety on the GPU (include/pom_batch.h PomMoveSafetySpec): every agent's six moves judged in one launch, byte-exact
against the compiled reference's answers (tests/golden/move_safety.npz), the checker (tests/move_safety_oracle.py: K x Oracle.step per
candidate, R as a boolean array) and the existing forecast, step and observation kernels; and the batch is left exactly as it was.
The states are played on the CPU and uploaded, so what the call has to say is known before the GPU runs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests.move_safety_oracle import at_horizon, move_safety

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "move_safety.npz")
KINDS = [("ffa", 57), ("stress", 23)]
SIZES = [5, 16, 67, 200]          # a short last tile, one whole tile, n no multiple of 4, several tiles
HORIZONS = [1, 4, 12, 32]
MASKS = [0xF, 0x1, 0xA]
SENTINEL = 0x55                   # no answer is 85: the ticks end at 32


@functools.lru_cache(maxsize=None)
def _played(kind, n, ticks):
    from tests.oracle_lib import Oracle
    s = FC.played_states(Oracle(), kind, n, ticks)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _full(kind, n, ticks, with_moves):
    """the checker's two outputs for all four agents at the longest horizon, computed once and shared (nobody writes to them), and
    the base moves; a shorter horizon's answers follow from them (at_horizon)"""
    from tests.oracle_lib import Oracle
    mv = FC.random_moves(n, 11 * n + 1) if with_moves else None
    death, escape = move_safety(Oracle(), _played(kind, n, ticks), 32, mv)
    for a in (death, escape):
        a.setflags(write=False)
    return death, escape, mv


def _want(kind, n, ticks, horizon, with_moves):
    death, escape, mv = _full(kind, n, ticks, with_moves)
    return at_horizon(death, horizon), at_horizon(escape, horizon), mv


def _invariants(death, escape):
    """the header's two consequences, and the dead rows"""
    assert ((death == -1) == (escape == -1)).all()
    assert (escape[death == 0] == 0).all()
    both = (death > 0) & (escape > 0)
    assert (escape[both] >= death[both]).all()


def _env(states, **kw):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    kw.setdefault("mode", MODE_ENV)
    env = BatchEnvironment(len(states), **kw)
    env.make_game(states)
    return env


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _same(got, want, what, mask=0xF, untouched=None):
    """both outputs equal the checker's in the rows of the mask; the other rows hold `untouched`"""
    rows = [a for a in range(4) if mask >> a & 1]
    others = [a for a in range(4) if not mask >> a & 1]
    for name, w in zip(("death_tick", "escape_tick"), want[:2]):
        if name not in got:
            continue
        g = got[name].cpu().numpy()
        bad = np.argwhere(g[:, rows] != w[:, rows])
        assert bad.size == 0, f"{what}: {name} differs in {len(bad)} places, first (env, row, move) {bad[0].tolist()}: got {g[:, rows][tuple(bad[0])]}, want {w[:, rows][tuple(bad[0])]}"
        if others:
            assert (g[:, others] == untouched).all(), f"{what}: {name}: a row outside the mask was written"


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
            got = env.move_safety(horizon, moves=_dev(g["moves"][ix]) if has_moves else None)
            _same(got, (g["death_tick"][ix], g["escape_tick"][ix]), f"horizon {horizon} moves {has_moves}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_move_safety_matches_the_checker(hip_lib, kind, ticks, n):
    """every horizon and mask, the others idle and with random first-tick moves; the outputs inside larger buffers of sentinels whose
    other bytes — the rows of the agents outside the mask among them — stay untouched; either output alone gives the same bytes"""
    import torch
    states = _played(kind, n, ticks)
    with _env(states) as env:
        before = env.get_state().tobytes()
        for horizon in HORIZONS:
            for with_moves in (False, True):
                want = _want(kind, n, ticks, horizon, with_moves)
                _invariants(*want[:2])
                for mask in MASKS:
                    bufs = [torch.full((8 + n * 24 + 64,), SENTINEL, dtype=torch.int8, device="cuda") for _ in range(2)]
                    assert all(b.data_ptr() % 8 == 0 for b in bufs)
                    out = {name: b[8:8 + n * 24].view(n, 4, 6) for name, b in zip(("death_tick", "escape_tick"), bufs)}
                    got = env.move_safety(horizon, agents=mask, moves=_dev(want[2]), out=out)
                    assert got["death_tick"].data_ptr() == out["death_tick"].data_ptr() and set(got) == set(out)
                    _same(got, want, f"{kind} n {n} horizon {horizon} moves {with_moves} mask {mask:#x}", mask, SENTINEL)
                    for b in bufs:
                        assert (b[:8] == SENTINEL).all() and (b[8 + n * 24:] == SENTINEL).all()
        assert env.get_state().tobytes() == before
        want = _want(kind, n, ticks, 12, True)
        for only, kw in (("death_tick", dict(escape=False)), ("escape_tick", dict(death=False))):
            got = env.move_safety(12, agents=[0, 2], moves=_dev(want[2]), **kw)
            assert set(got) == {only}
            _same(got, want, f"{only} alone", 0x5, -1)   # a tensor the call allocates: the rows not asked for are -1
        safe = env.safe_moves(12, moves=_dev(want[2]))
        assert safe.dtype == torch.bool and np.array_equal(safe.cpu().numpy(), want[1] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_bomb_is_usually_fatal_standing_and_usually_escapable(hip_lib, kind, ticks):
    """what the call is for, asserted on the checker's own answer before the GPU runs: of the live agents' BOMB candidates at horizon
    12 at least 100 die standing still yet have a way out, and at least 20 have none — a mask from death_tick alone would forbid the
    first group; then the GPU gives the same"""
    n, horizon = 67, 12
    want = _want(kind, n, ticks, horizon, False)
    death, escape = want[0][:, :, FC.B], want[1][:, :, FC.B]
    live = death >= 0
    assert int(((death > 0) & (escape == 0) & live).sum()) >= 100
    assert int((escape > 0).sum()) >= 20
    _invariants(*want[:2])
    with _env(_played(kind, n, ticks)) as env:
        _same(env.move_safety(horizon), want, f"{kind} BOMB")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_second_witness_for_death_tick_is_the_forecast(hip_lib, kind, ticks):
    """the 24 forecast calls of the recipe, the candidate written into the agent's column of the base moves: their
    agent_tick is death_tick"""
    import torch
    n, horizon = 67, 12
    base = _dev(FC.random_moves(n, 21))
    with _env(_played(kind, n, ticks)) as env:
        got = env.move_safety(horizon, moves=base, escape=False)["death_tick"]
        for a in range(4):
            for m in range(6):
                mv = base.clone()
                mv[:, a] = m
                tick = env.forecast(horizon, moves=mv)["agent_tick"][:, a]
                assert (got[:, a, m].to(torch.int32) == tick).all(), (a, m)
        assert int((got > 0).sum()) > n


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_second_witness_for_escape_tick_is_step_and_observe(hip_lib, kind, ticks):
    """the existing kernels as the yardstick: per variant a RAW twin is put back on the states and plays the candidate, then IDLE, with
    the code planes exported after every tick; Free is read off the board plane (0 passage, 6 7 8 the power-ups) and agent_attrs
    (x, y, alive), and R is grown in torch"""
    import torch
    from pomcpp_amd.batch import MODE_RAW
    n, horizon = 200, 12
    states = _played(kind, n, ticks)
    base = _dev(FC.random_moves(n, 5))
    idle = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    env_ix = torch.arange(n, device="cuda")

    def grow(r):
        g = r.clone()
        g[:, 1:, :] |= r[:, :-1, :]
        g[:, :-1, :] |= r[:, 1:, :]
        g[:, :, 1:] |= r[:, :, :-1]
        g[:, :, :-1] |= r[:, :, 1:]
        return g

    with _env(states) as env, _env(states, mode=MODE_RAW) as twin:
        got = env.move_safety(horizon, moves=base)
        _, attrs, _ = twin.observe(dtype="codes")
        dead0 = attrs[:, :, 2] == 0
        for a in range(4):
            for m in range(6):
                twin.make_game(states)
                first = base.clone()
                first[:, a] = m
                escape = torch.where(dead0[:, a], -1, 0).to(torch.int8)
                death = escape.clone()
                reach = torch.zeros((n, 11, 11), dtype=torch.bool, device="cuda")
                for t in range(1, horizon + 1):
                    twin.step_device(first if t == 1 else idle)
                    codes, attrs, _ = twin.observe(dtype="codes")
                    board = codes[:, 0]
                    alive = attrs[:, a, 2] != 0
                    own = torch.zeros_like(reach)
                    own[env_ix[alive], attrs[alive, a, 1].long(), attrs[alive, a, 0].long()] = True
                    free = (board == 0) | ((board >= 6) & (board <= 8)) | own
                    reach = own if t == 1 else grow(reach) & free
                    empty = ~reach.flatten(1).any(dim=1)
                    escape = torch.where((escape == 0) & empty, torch.full_like(escape, t), escape)
                    death = torch.where((death == 0) & ~alive, torch.full_like(death, t), death)
                assert (got["escape_tick"][:, a, m] == escape).all(), (a, m)
                assert (got["death_tick"][:, a, m] == death).all(), (a, m)
        assert int((got["escape_tick"] > 0).sum()) > 20


def _everything(env):
    """all the API can read of a handle"""
    out = dict(state=env.get_state().tobytes(), terminal=env.get_terminal_state().tobytes(), counters=env.counters().tolist(),
               episodes=env.episodes().tolist(), memory=env.policy_memory().tobytes(), chain=env.chain_stats())
    out.update({"status_" + k: v.tolist() for k, v in env.status().items()})
    out.update({"last_" + k: v.tolist() for k, v in env.last_results().items()})
    return out


@pytest.mark.gpu
def test_move_safety_leaves_no_trace(hip_lib):
    """an ENV-mode handle with end-of-tick resets and fresh boards, in the middle of SimpleAgent games: everything the API can read is
    the same before and after the calls, and 20 more ticks equal a twin's that never asked"""
    from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
    n, kw = 200, dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    with BatchEnvironment(n, **kw) as env, BatchEnvironment(n, **kw) as twin:
        for e in (env, twin):
            e.generate(9)
            e.step_simple(3, 40)
        before = _everything(env)
        assert _everything(twin) == before   # (both handles have now been read once: each settled its chained launches once)
        assert sum(before["last_finished"]) + sum(before["episodes"]) > 0 and before["counters"][0] == n * 40
        for horizon, agents, mv in ((12, None, _dev(FC.random_moves(n, 1))), (32, [1], None), (1, 0xA, _dev(FC.random_moves(n, 2)))):
            got = env.move_safety(horizon, agents=agents, moves=mv)
            assert int((got["death_tick"] > 0).sum()) > 0 or horizon == 1
            assert _everything(env) == before, horizon
        env.step_simple(3, 20)
        env.move_safety(8)
        twin.step_simple(3, 20)
        assert _everything(env) == _everything(twin)


@pytest.mark.gpu
def test_move_safety_after_chained_launches_settles(hip_lib, oracle):
    """20 chained ticks, then the call with nothing in between: it starts from the state a download returns"""
    from pomcpp_amd.batch import DIST_RANDOM, ISSUE_CHAIN, MODE_ENV
    n = 600
    with _env(_played("stress", n, 23), mode=MODE_ENV, auto_reset=True, max_steps=300, issue_mode=ISSUE_CHAIN) as env:
        assert env.issue_info()[0] == "chain"
        env.step_random(5, DIST_RANDOM, ticks=20)
        launches = env.chain_stats()["launches"]
        got = env.move_safety(12)
        assert launches == 20 and env.chain_stats()["launches"] == 20
        _same(got, move_safety(oracle, env.get_state(), 12), "after 20 chained ticks")


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", [(16, 1), (32, 1), (64, 1)])
def test_handle_shapes_give_the_same_bytes(hip_lib, epw, lpe):
    """the call's own launch shape does not depend on the handle's: the device buffers are 16-env tiles whatever the shape"""
    n = 67
    want = _want("stress", n, 23, 12, True)
    with _env(_played("stress", n, 23), envs_per_wave=epw, lanes_per_env=lpe) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        _same(env.move_safety(12, moves=_dev(want[2])), want, f"epw {epw}")


@pytest.mark.gpu
def test_rows_do_not_depend_on_the_wavefront_mates(hip_lib, oracle):
    """every actor of tests/tile_mates.py (deep chains, claim-map victims, bounce chains, queue limits) in each of the 16 columns of a
    tile of its own, the other 15 columns played stress boards: its rows are the checker's solo rows, wherever it sits and whoever
    sits beside it — the tile stays in LDS for 16 ticks, the scratch rows are never re-initialised, and the quads of a wavefront leave
    the loop at different ticks"""
    from tests import tile_mates as TM
    entries = TM.actors(oracle)
    A, horizon = len(entries), TM.TICKS
    start = np.concatenate([e.start for e in entries])
    first = np.stack([e.moves[0] for e in entries]).astype(np.int32)
    want = move_safety(oracle, start, horizon, first)
    assert int((want[0] > 0).sum()) > 100 and (want[1] > 0).any()   # the actors' agents die, and some have nowhere to go
    mates = _played("stress", 240, 23)
    who = np.repeat(np.arange(A), 16)                    # tile k: actor k // 16 ...
    col = np.tile(np.arange(16), A)                      # ... in column k % 16
    n = A * 16 * 16
    states = mates[np.arange(n) % mates.size].copy()
    moves = FC.random_moves(n, 3)
    at = np.arange(A * 16) * 16 + col
    states[at], moves[at] = start[who], first[who]
    with _env(states) as env:
        got = env.move_safety(horizon, moves=_dev(moves))
        sel = _dev(at.astype(np.int64))
        picked = {k: v[sel] for k, v in got.items()}
        _same(picked, (want[0][who], want[1][who]), "actors among stress mates")


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header, with the call's name in the message, and nothing written"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _MoveSafetySpec
    n = 32
    with _env(_played("ffa", 67, 57)[:n].copy()) as env:
        lib, h = env._lib, env._h
        dbuf = torch.full((n * 24 + 64,), SENTINEL, dtype=torch.int8, device="cuda")
        xbuf = torch.full((n * 24 + 64,), SENTINEL, dtype=torch.int8, device="cuda")
        mv = torch.zeros((n * 4 + 16,), dtype=torch.int32, device="cuda")
        size, d, x, m = C.sizeof(_MoveSafetySpec), dbuf.data_ptr(), xbuf.data_ptr(), mv.data_ptr()
        bad = {
            "struct_size": _MoveSafetySpec(size - 8, 4, 15, 0, None, d, x, 0),
            "horizon 0": _MoveSafetySpec(size, 0, 15, 0, None, d, x, 0),
            "horizon 33": _MoveSafetySpec(size, 33, 15, 0, None, d, x, 0),
            "agent_mask 0": _MoveSafetySpec(size, 4, 0, 0, None, d, x, 0),
            "agent_mask 16": _MoveSafetySpec(size, 4, 16, 0, None, d, x, 0),
            "agent_mask -1": _MoveSafetySpec(size, 4, -1, 0, None, d, x, 0),
            "reserved_": _MoveSafetySpec(size, 4, 15, 1, None, d, x, 0),
            "reserved2_": _MoveSafetySpec(size, 4, 15, 0, None, d, x, 1),
            "both outputs null": _MoveSafetySpec(size, 4, 15, 0, m, None, None, 0),
            "death_tick + 4": _MoveSafetySpec(size, 4, 15, 0, None, d + 4, x, 0),
            "escape_tick + 1": _MoveSafetySpec(size, 4, 15, 0, None, None, x + 1, 0),
            "moves + 2": _MoveSafetySpec(size, 4, 15, 0, m + 2, d, x, 0),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_move_safety(h, C.byref(spec)))
            assert err.value.code == 1 and "pom_batch_move_safety" in str(err.value), what
        good = _MoveSafetySpec(size, 4, 15, 0, None, d, x, 0)
        for call in (lambda: lib.pom_batch_move_safety(None, C.byref(good)), lambda: lib.pom_batch_move_safety(h, None)):
            with pytest.raises(PomError) as err:
                _check(lib, call())
            assert err.value.code == 1 and "pom_batch_move_safety" in str(err.value)
        env.sync()
        assert (dbuf == SENTINEL).all() and (xbuf == SENTINEL).all()
        assert env.get_state().tobytes() == before
        for kw in (dict(horizon=0), dict(horizon=33), dict(horizon=4, agents=16), dict(horizon=4, agents=[4]), dict(horizon=4, agents=[]),
                   dict(horizon=4, death=False, escape=False), dict(horizon=4, moves=mv[:n * 4].view(n, 4).to(torch.int64)),
                   dict(horizon=4, out={"death_tick": dbuf[:n * 24].view(n, 24)}),
                   dict(horizon=4, out={"escape_tick": xbuf[:n * 24].view(n, 4, 6).to(torch.int32)})):
            with pytest.raises(ValueError):
                env.move_safety(**kw)
        # moves_dev needs 4-byte and the outputs 8-byte alignment only: a call 4 and 8 bytes into the buffers runs
        _check(lib, lib.pom_batch_move_safety(h, C.byref(_MoveSafetySpec(size, 4, 15, 0, m + 4, d + 8, x + 8, 0))))
        env.sync()
        assert not (dbuf[8:8 + n * 24] == SENTINEL).any() and not (xbuf[8:8 + n * 24] == SENTINEL).any()
        assert (dbuf[:8] == SENTINEL).all() and (dbuf[8 + n * 24:] == SENTINEL).all()
