"""The quad tick with one live agent word per lane (pom_step_body.h: `mine_`, owner_lanes_begin / owner_lanes_end): lane m of an env's
quad carries agent m's word through the whole tick, "agent id" is a predicate on the lane number (kill, kill_set,
owner_bombcount_dec), a look at another agent's word a quad reduction (get_agent, agent_word), and the four lanes get identical
words again once, at the end of the tick.  A wrong lane's word shows as a wrong bombCount, a wrong dead flag or a wrong alive count
of ONE agent of one env, so the check is every byte of every env after every tick.

300 ticks of step_random, one tick per call, the quad shape <16, 4> against the oracle after every tick, and at the end against
the one-lane shape <16, 1> (which keeps the replicated words) playing the same 300 ticks: states, sticky UB flags, counters.
(The one-lane shape exists for the start-of-tick reset only; against the end-of-tick run it is compared with the games that
ended on the last tick put back on their start states, and without the restart counter, which is one restart ahead there.)
Sizes: 16 envs (one tile: one wavefront, 64 agents) and 40 (three tiles, the last with 8 envs and 8 columns of padding: 32 invalid
lanes).  Boards: ffa with uniform moves, stress with the stress mix.  Both reset modes.  Episodes are capped at CAP ticks so that
restarts happen on every board kind.

The seeds (RUNS) were chosen on the CPU with the oracle so that each of the cases the predicated updates have to get right occurs
in those ticks — on the stress boards every one of them in the first 16 envs already, which are the one-tile run; on the ffa
boards all but the last (nobody can kick when an ffa game starts, and of 36 seed pairs tried none had a kick beside a pick-up).
test_the_runs_contain_the_cases recounts them; the counts (ticks x envs in which the case occurs; first 16 envs / all 40):

  case                                                      ffa            stress
  two top explosions, different owners                        45 / 124     610 / 1289
  a blast kills its own owner                                418 / 982     421 / 917
  a blast whose owner is already dead                          4 / 10      288 / 804
  a chained blast kills two agents                             1 / 1       143 / 308
  a kick and a power-up pick-up in one tick                    0 / 0         1 / 1

How a case is recognised from the oracle's states before and after a tick (conservative: what counts is certainly the case):
  - two top explosions: the two bombs at the head of the queue have timer 1 (both run out this tick and are popped by TickBombs'
    loop, step_utility.cpp:233-244), different owners, and neither lies in the other's row or column (so the second is not set off
    by the first's flame: it IS a second top explosion);
  - own owner: the head bomb has timer 1, its owner is alive before the tick, dead after it, and ends the tick on the blast's
    cross (same row or column, within the bomb's strength);
  - dead owner: the head bomb has timer 1 and its owner is dead before the tick;
  - chained, two dead: the alive count falls by two or more in a tick in which more bombs leave the queue than had timer 1 (bombs
    planted this tick only hide departures), i.e. some bomb went off by another's flame;
  - kick and pick-up: a live agent that can kick ends the tick on a cell that showed Item::BOMB before it and on which a bomb was
    queued, and some agent's maxBombCount, bombStrength or canKick rises in the same tick."""
import numpy as np
import pytest

import pomcpp_amd as pa
import pomcpp_amd.state as S
from pomcpp_amd.state import Item

TICKS, CAP, N_MAX, TILE = 300, 120, 40, 16
DIST_RANDOM, DIST_STRESS = 1, 2  # (pomcpp_amd.batch's constants; the module is not imported where there is no library)
#        kind      move mix     board seed  move seed
RUNS = {"ffa": (DIST_RANDOM, 4, 2), "stress": (DIST_STRESS, 1, 5)}
CASES = ("two_tops", "own_owner", "dead_owner", "chain_two_dead", "kick_and_pickup")

_traces = {}


def trace(oracle, kind):
    """start states and the oracle's states after each tick (start-of-tick restarts, as pom_oracle_run_random plays): computed once
    per board kind, shared by every test, never changed"""
    if kind not in _traces:
        dist, board_seed, seed = RUNS[kind]
        start = pa.make_boards(N_MAX, seed=board_seed, kind=kind)
        after = np.zeros((TICKS, N_MAX), dtype=start.dtype)
        cur = start.copy()
        for t in range(TICKS):
            oracle.run_random(cur, start, 1, seed, 0, t, dist, CAP)
            after[t] = cur
        after["agents"]["pad"] = 0
        for a in (start, after):
            a.setflags(write=False)
        _traces[kind] = (start, after)
    return _traces[kind]


def finished(states):
    return (states["aliveAgents"] <= 1) | (states["timeStep"] >= CAP)


def count_cases(start, after):
    """per case, the number of (tick, env) pairs in which it occurs: [first TILE envs, all envs]"""
    counts = {c: [0, 0] for c in CASES}
    prev = start.copy()
    for t in range(after.shape[0]):
        done = finished(prev)
        before = prev.copy()
        before[done] = start[done]  # what the tick was played on
        for e in range(before.size):
            b, a = before[e], after[t, e]
            nb = int(b["bombs_count"])
            bombs = [int(S.queue_get(b, "bombs", k)) for k in range(nb)]
            hit = set()
            ripe = [w for w in bombs if S.bomb_time(w) == 1]
            if nb >= 2 and S.bomb_time(bombs[0]) == 1 and S.bomb_time(bombs[1]) == 1 and S.bomb_id(bombs[0]) != S.bomb_id(bombs[1]) \
                    and S.bomb_x(bombs[0]) != S.bomb_x(bombs[1]) and S.bomb_y(bombs[0]) != S.bomb_y(bombs[1]):
                hit.add("two_tops")
            if nb >= 1 and S.bomb_time(bombs[0]) == 1:
                w = bombs[0]
                o = S.bomb_id(w)
                if o < 4 and b["agents"][o]["dead"]:
                    hit.add("dead_owner")
                if o < 4 and not b["agents"][o]["dead"] and a["agents"][o]["dead"]:
                    dx, dy = int(a["agents"][o]["x"]) - S.bomb_x(w), int(a["agents"][o]["y"]) - S.bomb_y(w)
                    if (dx == 0 or dy == 0) and abs(dx) + abs(dy) <= S.bomb_strength(w):
                        hit.add("own_owner")
            if int(b["aliveAgents"]) - int(a["aliveAgents"]) >= 2 and nb - int(a["bombs_count"]) > len(ripe):
                hit.add("chain_two_dead")
            ag_b, ag_a = b["agents"], a["agents"]
            pickup = bool(((ag_a["maxBombCount"] > ag_b["maxBombCount"]) | (ag_a["bombStrength"] > ag_b["bombStrength"]) |
                           (ag_a["canKick"] > ag_b["canKick"])).any())
            kick = False
            for i in range(4):
                if ag_b[i]["dead"] or not ag_b[i]["canKick"]:
                    continue
                x, y = int(ag_a[i]["x"]), int(ag_a[i]["y"])
                if (x, y) != (int(ag_b[i]["x"]), int(ag_b[i]["y"])) and b["board"][y, x] == Item.BOMB \
                        and any((S.bomb_x(w), S.bomb_y(w)) == (x, y) for w in bombs):
                    kick = True
            if kick and pickup:
                hit.add("kick_and_pickup")
            for c in hit:
                counts[c][0] += e < TILE
                counts[c][1] += 1
        prev = after[t]
    return counts


_counts = {}


def counts_of(oracle, kind):
    if kind not in _counts:
        _counts[kind] = count_cases(*trace(oracle, kind))
    return _counts[kind]


@pytest.mark.parametrize("kind", sorted(RUNS))
def test_the_runs_contain_the_cases(oracle, kind):
    start, after = trace(oracle, kind)
    counts = counts_of(oracle, kind)
    print(kind, counts)
    assert counts == EXPECTED_COUNTS[kind], counts  # the docstring's table
    restarts = sum(int(finished(after[t][:TILE]).sum()) for t in range(TICKS))
    assert restarts > 0, "no game of the first tile ends: the reset modes would be the same run"


EXPECTED_COUNTS = {"ffa": {'two_tops': [45, 124], 'own_owner': [418, 982], 'dead_owner': [4, 10], 'chain_two_dead': [1, 1], 'kick_and_pickup': [0, 0]},
                   "stress": {'two_tops': [610, 1289], 'own_owner': [421, 917], 'dead_owner': [288, 804], 'chain_two_dead': [143, 308], 'kick_and_pickup': [1, 1]}}


def test_every_case_occurs_in_one_tile(oracle):
    """each case at least once within the first 16 envs: every one of them on the stress boards, all but the kick beside a pick-up on
    the ffa boards"""
    stress, ffa = (counts_of(oracle, kind) for kind in ("stress", "ffa"))
    assert all(tile > 0 for tile, _all in stress.values()), stress
    assert all(tile > 0 for c, (tile, _all) in ffa.items() if c != "kick_and_pickup"), ffa


@pytest.mark.gpu
@pytest.mark.parametrize("reset", ["at_start", "at_end"])
@pytest.mark.parametrize("n", [TILE, N_MAX])
@pytest.mark.parametrize("kind", sorted(RUNS))
def test_quad_tick_every_tick_against_the_oracle_and_the_one_lane_shape(hip_lib, oracle, kind, n, reset):
    from pomcpp_amd.batch import CNT_EPISODES, CNT_STEPS, MODE_ENV, RESET_AT_END, RESET_AT_START, BatchEnvironment
    dist, _board_seed, seed = RUNS[kind]
    start_all, after = trace(oracle, kind)
    start = np.ascontiguousarray(start_all[:n])
    at_end = reset == "at_end"
    mode = RESET_AT_END if at_end else RESET_AT_START
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=mode, max_steps=CAP, envs_per_wave=16, lanes_per_env=4) as env:
        assert env.launch_shape()[:2] == (16, 4)
        env.make_game(start)
        for t in range(TICKS):
            env.step_random(seed, dist, ticks=1)
            want = after[t, :n].copy()
            if at_end:  # the tick that ends a game leaves the env on its start state
                done = finished(want)
                want[done] = start[done]
            got = env.get_state()
            if got.tobytes() != want.tobytes():
                bad = np.nonzero((got.view(np.uint8).reshape(n, -1) != want.view(np.uint8).reshape(n, -1)).any(axis=1))[0]
                fields = [f for f in got.dtype.names if got[f][bad[0]].tobytes() != want[f][bad[0]].tobytes()]
                raise AssertionError(f"tick {t}: envs {bad.tolist()} differ from the oracle; env {int(bad[0])} in {fields}")
        quad = (env.get_state(), env.status()["ubflags"].copy(), env.counters().copy())
    # the one-lane shape is built for the start-of-tick reset only: the same games, a game that ended with the last tick still
    # standing on its final state (the end-of-tick mode is one restart ahead there, and in its restart counter)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=CAP, envs_per_wave=16, lanes_per_env=1) as env:
        assert env.launch_shape()[:2] == (16, 1)
        env.make_game(start)
        env.step_random(seed, dist, ticks=TICKS)
        one = (env.get_state(), env.status()["ubflags"].copy(), env.counters().copy())
    want = one[0].copy()
    if at_end:
        done = finished(want)
        want[done] = start[done]
    assert quad[0].tobytes() == want.tobytes(), "the quad shape and the one-lane shape end on different states"
    assert np.array_equal(quad[1], one[1])
    same = slice(None) if not at_end else [CNT_STEPS, CNT_EPISODES]
    assert np.array_equal(quad[2][same], one[2][same]), (quad[2], one[2])
