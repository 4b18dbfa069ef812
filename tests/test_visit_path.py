"""The step kernels' path AROUND the tick: restarts (snapshot records, fresh boards, the end-of-tick reset; the register rows are
unpacked once, behind the restarts), the move pick (a wave-uniform branch on the distribution and on explicit moves), the counters
and the record's top bytes (queue indices and counts, status, UB flags), each against a replay on the oracle.

Shapes: n = 16 (one tile), 40 (a short last tile: padding lanes that must neither restart nor count), 144 (nine tiles: more than one
per XCD).  The replay is Oracle.step per env and tick with the moves of pom_rng_moves (tests/rollout_oracle.py restates the stream), under
Environment::Step's bookkeeping; it is checked against Oracle.run_random where that exists, and it counts what counters() reports:
[steps, episodes finished, resets, ticks that raised a UB flag]."""
import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import (BatchEnvironment, MODE_ENV, DIST_HARMLESS, DIST_RANDOM, DIST_STRESS, RESET_AT_START, RESET_AT_END)
from tests import rollout_oracle as RO

pytestmark = pytest.mark.gpu

SHAPES = (16, 40, 144)
TICKS = 40
ENV_OFFSET, TICK0, SEED, BSEED = 1000, 7, 23, 5


def _clean(states):
    out = states.copy()
    out["agents"]["pad"] = 0
    return out


def _same(got, want, what):
    want = _clean(want)
    if got.tobytes() != want.tobytes():
        g, w = got.view(np.uint8).reshape(got.size, -1), want.view(np.uint8).reshape(want.size, -1)
        bad = np.nonzero((g != w).any(axis=1))[0]
        e = int(bad[0])
        fields = [f for f in got.dtype.names if got[e][f].tobytes() != want[e][f].tobytes()]
        raise AssertionError(f"{what}: {bad.size} of {got.size} envs differ, first env {e}, fields {fields}")


def _finished(s, cap):
    return (s["aliveAgents"] <= 1) | ((cap > 0) & (s["timeStep"] >= cap))


def replay(oracle, start, ticks, dist, cap, *, snapshot=None, fresh=False, at_end=False, env_offset=ENV_OFFSET, tick0=TICK0, seed=SEED,
           moves_out=None):
    """-> (states after every tick, counters after every tick, UB flags raised per tick [ticks, n]).  Start-of-tick reset: a finished env
    restarts (from `snapshot`, or with `fresh` on its next board) before its tick; `at_end`: right after the tick that finished it."""
    n = start.size
    s = start.copy()
    snap = start if snapshot is None else snapshot
    episodes = np.zeros(n, dtype=np.int64)
    cnt = np.zeros(4, dtype=np.int64)
    states, counters, flags = [], [], np.zeros((ticks, n), dtype=np.uint32)

    def restart(e):
        if fresh:
            episodes[e] += 1
            s[e] = oracle.boardgen(BSEED, [env_offset + e], [episodes[e]])[0]
        else:
            s[e] = snap[e]
        cnt[2] += 1

    for t in range(ticks):
        for e in range(n):
            if not at_end and _finished(s[e:e + 1], cap)[0]:
                restart(e)
            mv = RO.rng_moves(seed, env_offset + e, tick0 + t, dist)
            if moves_out is not None:
                moves_out[t, e] = mv
            flags[t, e] = oracle.step(s[e:e + 1], mv)
            s["timeStep"][e] += 1
            cnt[0] += 1
            cnt[3] += flags[t, e] != 0
            if _finished(s[e:e + 1], cap)[0]:
                cnt[1] += 1
                if at_end:
                    restart(e)
        states.append(s.copy())
        counters.append(cnt.copy())
    return states, counters, flags


def burned_in(oracle, n, seed, kind="ffa", dist=DIST_RANDOM, ticks=60):
    """boards with `ticks` ticks of random play (restarts included) behind them: games of every age, none of them finished"""
    start = pa.make_boards(n, seed=seed, kind=kind)
    s = start.copy()
    oracle.run_random(s, start, ticks, 77, 0, 0, dist, 800)
    over = _finished(s, 800)
    s[over] = start[over]  # (a finished upload would be its own finished snapshot)
    return _clean(s)


# ---- restart storms -------------------------------------------------------------------------------------------------------------
STORMS = [(n, cap) for n in SHAPES for cap in (2, 3)] + [(n, 800) for n in SHAPES]
_storm_cache = {}


def _storm(oracle, n, cap):
    """the boards and the oracle's replay of a storm case, computed once and shared (never changed)"""
    key = (n, cap)
    if key not in _storm_cache:
        start = _clean(pa.make_boards(n, seed=41 + n)) if cap != 800 else burned_in(oracle, n, 41 + n)
        states, counters, flags = replay(oracle, start, TICKS, DIST_RANDOM, cap)
        want = start.copy()
        steps = oracle.run_random(want, start, TICKS, SEED, ENV_OFFSET, TICK0, DIST_RANDOM, cap)
        assert steps == n * TICKS and _clean(want).tobytes() == _clean(states[-1]).tobytes(), "the replay is not Oracle.run_random"
        if cap != 800:  # every env restarts on the same ticks: 16 restarts in one visit of a tile
            assert counters[-1][2] == n * ((TICKS - 1) // cap)
        else:  # a few restarts a visit, as they come
            assert 0 < counters[-1][2] < n * TICKS // 4
        _storm_cache[key] = (start, states, counters)
    return _storm_cache[key]


def _env(n, cap, reset=RESET_AT_START, **kw):
    return BatchEnvironment(n, mode=MODE_ENV, auto_reset=reset, max_steps=cap, env_offset=ENV_OFFSET, **kw)


@pytest.mark.parametrize("n,cap", STORMS)
def test_restart_storm_chained_call(hip_lib, oracle, n, cap):
    start, states, counters = _storm(oracle, n, cap)
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        env.step_random(SEED, DIST_RANDOM, ticks=TICKS)
        _same(env.get_state(), states[-1], f"n {n} cap {cap} after {TICKS} ticks")
        assert env.counters().tolist() == counters[-1].tolist()


@pytest.mark.parametrize("n,cap", STORMS)
def test_restart_storm_one_tick_per_call(hip_lib, oracle, n, cap):
    start, states, counters = _storm(oracle, n, cap)
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        for t in range(TICKS):
            env.step_random(SEED, DIST_RANDOM, ticks=1)
            _same(env.get_state(), states[t], f"n {n} cap {cap} tick {t}")
            assert env.counters().tolist() == counters[t].tolist(), t


@pytest.mark.parametrize("n,cap", STORMS)
def test_restart_storm_four_ticks_per_launch(hip_lib, oracle, n, cap):
    start, states, counters = _storm(oracle, n, cap)
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        for t in range(3, TICKS, 4):
            env.step_random(SEED, DIST_RANDOM, ticks=4, ticks_per_launch=4)
            _same(env.get_state(), states[t], f"n {n} cap {cap} tick {t}")
            assert env.counters().tolist() == counters[t].tolist(), t


_fresh_cache = {}


def _fresh_storm(oracle, n, cap):
    """the same storms with a new board per game: generated boards for the caps 2 and 3; for the natural restarts (cap 800) the burned-in
    boards of the snapshot storms, uploaded — generated boards would not finish a game within the ticks played — whose games end on
    board (BSEED, env, 1).  Computed once and shared."""
    key = (n, cap)
    if key not in _fresh_cache:
        start = oracle.boardgen(BSEED, np.arange(n) + ENV_OFFSET, np.zeros(n)) if cap != 800 else burned_in(oracle, n, 41 + n)
        states, counters, _ = replay(oracle, start, TICKS, DIST_RANDOM, cap, fresh=True)
        want, eps = start.copy(), np.zeros(n, dtype=np.int32)
        steps = oracle.run_random_fresh(want, eps, TICKS, SEED, BSEED, ENV_OFFSET, TICK0, DIST_RANDOM, cap)
        assert steps == n * TICKS and _clean(want).tobytes() == _clean(states[-1]).tobytes(), "the replay is not Oracle.run_random_fresh"
        assert counters[-1][2] == eps.sum() > 0
        _fresh_cache[key] = (start, states, counters, eps)
    return _fresh_cache[key]


@pytest.mark.parametrize("path", ["chained", "one_tick_per_call", "four_ticks_per_launch"])
@pytest.mark.parametrize("n,cap", STORMS)
def test_restart_storm_fresh_boards(hip_lib, oracle, n, cap, path):
    start, states, counters, eps = _fresh_storm(oracle, n, cap)
    with _env(n, cap, fresh_boards=True, board_seed=BSEED) as env:
        if cap != 800:
            env.generate(BSEED)
            _same(env.get_state(), start, "generated boards")
        else:
            env.make_game(start)
        env.set_tick(TICK0)
        if path == "chained":
            env.step_random(SEED, DIST_RANDOM, ticks=TICKS)
        elif path == "one_tick_per_call":
            for t in range(TICKS):
                env.step_random(SEED, DIST_RANDOM, ticks=1)
                _same(env.get_state(), states[t], f"fresh boards, n {n} cap {cap} tick {t}")
                assert env.counters().tolist() == counters[t].tolist(), t
        else:
            for t in range(3, TICKS, 4):
                env.step_random(SEED, DIST_RANDOM, ticks=4, ticks_per_launch=4)
                _same(env.get_state(), states[t], f"fresh boards, n {n} cap {cap} tick {t}")
                assert env.counters().tolist() == counters[t].tolist(), t
        _same(env.get_state(), states[-1], f"fresh boards, n {n} cap {cap}, {path}")
        assert env.counters().tolist() == counters[-1].tolist()
        assert env.episodes().tolist() == eps.tolist()


@pytest.mark.parametrize("n,cap", STORMS)
def test_restart_storm_reset_at_end_through_step_device(hip_lib, oracle, n, cap):
    """the end-of-tick reset: the final records go to the terminal buffer, the envs restart from their snapshot records in the same visit"""
    import torch
    start, _, _ = _storm(oracle, n, cap)
    moves = np.zeros((TICKS, n, 4), dtype=np.int32)
    states, counters, _ = replay(oracle, start, TICKS, DIST_RANDOM, cap, at_end=True, moves_out=moves)
    with _env(n, cap, reset=RESET_AT_END) as env:
        env.make_game(start)
        for t in range(TICKS):
            env.step_device(torch.from_numpy(moves[t]).to("cuda"))
            _same(env.get_state(), states[t], f"reset at end, n {n} cap {cap} tick {t}")
            assert env.counters().tolist() == counters[t].tolist(), t
        assert not env.status()["done"].any()


# ---- the move pick --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dist", [DIST_HARMLESS, DIST_RANDOM, DIST_STRESS])
def test_move_pick_drawn_and_explicit(hip_lib, oracle, dist):
    """64 ticks from fixed boards: the device's draw of every distribution = pom_rng_moves on the host, and the same moves handed over
    as a tape (the other side of the kernel's branch on explicit moves) play the same games"""
    import torch
    n, ticks, cap = 40, 64, 800
    start = _clean(pa.make_boards(n, seed=3, kind="stress" if dist == DIST_STRESS else "ffa"))
    tape = np.zeros((ticks, n, 4), dtype=np.int32)
    states, counters, _ = replay(oracle, start, ticks, dist, cap, moves_out=tape)
    want = start.copy()
    oracle.run_random(want, start, ticks, SEED, ENV_OFFSET, TICK0, dist, cap)
    assert _clean(want).tobytes() == _clean(states[-1]).tobytes(), "the replay is not Oracle.run_random"
    assert set(np.unique(tape).tolist()) == set(range(5 if dist == DIST_HARMLESS else 6)), "every move of the distribution occurs"
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        for t in range(ticks):
            env.step_random(SEED, dist, ticks=1)
            _same(env.get_state(), states[t], f"dist {dist} tick {t}")
        drawn, drawn_cnt = env.get_state(), env.counters()
    assert drawn_cnt.tolist() == counters[-1].tolist()
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        env.step_random(SEED, dist, ticks=ticks)  # the chained call
        assert env.get_state().tobytes() == drawn.tobytes() and env.counters().tolist() == drawn_cnt.tolist()
    with _env(n, cap) as env:
        env.make_game(start)
        env.step_device_many(torch.from_numpy(tape).to("cuda"))
        assert env.get_state().tobytes() == drawn.tobytes(), f"dist {dist}: the tape's games are not the drawn games"
        assert env.counters().tolist() == drawn_cnt.tolist()


# ---- the counters ---------------------------------------------------------------------------------------------------------------
UB_SEED = 9  # stress boards of this seed raise UB flags on the oracle within the ticks played (asserted below)


def test_counters_with_ub_ticks_and_padding(hip_lib, oracle):
    """stress boards and the stress distribution on a short last tile: all four counters move, UB ticks included"""
    n, ticks, cap = 40, TICKS, 30
    start = burned_in(oracle, n, UB_SEED, kind="stress", dist=DIST_STRESS, ticks=25)
    states, counters, flags = replay(oracle, start, ticks, DIST_STRESS, cap)
    assert counters[-1][3] >= 1, "precondition: the oracle reports at least one UB tick on these boards"
    assert counters[-1][1] >= 1 and counters[-1][2] >= 1
    for tpl in (1, 4):
        with _env(n, cap) as env:
            env.make_game(start)
            env.set_tick(TICK0)
            env.step_random(SEED, DIST_STRESS, ticks=ticks, ticks_per_launch=tpl)
            _same(env.get_state(), states[-1], f"stress, {tpl} ticks per launch")
            assert env.counters().tolist() == counters[-1].tolist(), tpl
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        for t in range(ticks):
            env.step_random(SEED, DIST_STRESS, ticks=1)
            assert env.counters().tolist() == counters[t].tolist(), t


@pytest.mark.parametrize("n", SHAPES)
def test_counters_with_nothing_to_add(hip_lib, oracle, n):
    """harmless moves, no cap: nobody finishes, restarts or raises a flag — three of the four addends are 0 for whole launches; and a
    launch over finished envs without auto-reset adds nothing at all"""
    start = _clean(pa.make_boards(n, seed=8))
    states, counters, _ = replay(oracle, start, 8, DIST_HARMLESS, 0)
    assert counters[-1].tolist() == [8 * n, 0, 0, 0]
    with _env(n, 0) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        for t in range(8):
            env.step_random(SEED, DIST_HARMLESS, ticks=1)
            assert env.counters().tolist() == counters[t].tolist()
        _same(env.get_state(), states[-1], "harmless")
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=False, max_steps=1, env_offset=ENV_OFFSET) as env:
        env.make_game(start)
        env.step_random(SEED, DIST_HARMLESS, ticks=1)
        assert env.counters().tolist() == [n, n, 0, 0]  # everybody played one tick and ran into the cap
        env.step_random(SEED, DIST_HARMLESS, ticks=3)
        assert env.counters().tolist() == [n, n, 0, 0]  # finished envs are left alone: every addend 0


# ---- the top bytes of the agent words -------------------------------------------------------------------------------------------
def test_top_bytes_survive_a_tick(hip_lib, oracle):
    """upload -> 1 tick -> download: bombs.index / count, flames.index / count, aliveAgents come back as the oracle has them; status and
    the 16 UB flags (which only ticks can set) are followed over ticks in which some envs restart and others do not"""
    n, cap = 40, 30
    start = burned_in(oracle, n, UB_SEED, kind="stress", dist=DIST_STRESS, ticks=25)
    for f in ("bombs_index", "bombs_count", "flames_index", "flames_count"):
        assert (start[f] != 0).any(), f"precondition: some env uploads a non-zero {f}"
    assert len(set(start["aliveAgents"].tolist())) > 1
    one, _, _ = replay(oracle, start, 1, DIST_STRESS, cap)
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        env.step_random(SEED, DIST_STRESS, ticks=1)
        _same(env.get_state(), one[0], "upload, one tick, download")
    ticks = TICKS
    states, counters, flags = replay(oracle, start, ticks, DIST_STRESS, cap)
    sticky = np.zeros(n, dtype=np.uint32)
    seen_kept = seen_restart = False
    with _env(n, cap) as env:
        env.make_game(start)
        env.set_tick(TICK0)
        prev = start
        for t in range(ticks):
            restarted = _finished(prev, cap)  # these envs began the tick from their snapshot record: flags clear
            seen_restart |= bool((restarted & (sticky != 0)).any())
            seen_kept |= bool((~restarted & (sticky != 0)).any())
            sticky = np.where(restarted, 0, sticky).astype(np.uint32) | flags[t]
            env.step_random(SEED, DIST_STRESS, ticks=1)
            st = env.status()
            _same(env.get_state(), states[t], f"tick {t}")
            assert st["ubflags"].tolist() == sticky.tolist(), t
            assert st["done"].astype(bool).tolist() == _finished(states[t], cap).tolist(), t
            assert st["time_step"].tolist() == states[t]["timeStep"].tolist() and st["alive"].tolist() == states[t]["aliveAgents"].tolist()
            prev = states[t]
    assert seen_kept, "precondition: some env carried UB flags through a tick in which it did not restart"
    assert seen_restart, "precondition: some env with UB flags set restarted"
