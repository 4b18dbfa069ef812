"""What the inputs of tests/test_gpu_mates_queries.py reach (tests/mates_queries.py), recounted without a GPU, so that a change of the
actors, the compositions or the checkers is noticed here and not as a GPU test that quietly checks less.

The mixed step puts SimpleAgents into the actors' seats.  The actors are built so that this does not disarm them: on their decisive
ticks nothing an agent does reaches the bombs.  Under masks 0b0110 and 0xF the bomb queue, bombs_count and flames_count of every env
equal its actor's solo trace after ticks 0, 1, 2 and 3 for all 18 deep_b, all 12 deep_top and all 63 select actors, in every env that
holds one; for claims_full after tick 0, its decisive one (after tick 1 still in 335 of its 412 envs: from then on the agents, whose
draws are keyed by the env, walk into its bombs' ways).  bounce_H depends on the scripted agent moves — the kicker's step IS the event —
so under a mask 6 of the 7 diverge: mask 0, the scripts through the mixed kernel, is what exercises them."""
import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import edge_queries as EQ
from tests import mates_queries as MQ
from tests import tile_mates as TM
from tests.edge_states import FATAL, UB_FLAME_QUEUE_RANGE
from tests.range_model import RESET_AT_END, RESET_AT_START


@pytest.fixture(scope="module")
def mates(oracle):
    return MQ.mates(oracle)


def test_the_batch_is_the_mates_modules_families(mates):
    cast = mates.stage.cast
    fams = [("overlay", TM.overlay(cast, 16)[0]), ("pairs", TM.pairs(cast, 16)), ("restart", TM.restart(cast, 16)), ("crowd_tail5", TM.crowd(cast, 16, 5))]
    assert [f[1].size for f in fams] == [1440, 1536, 160, 245]
    assert np.array_equal(mates.who, np.concatenate([f[1] for f in fams])) and mates.fam == sum(([f[0]] * f[1].size for f in fams), [])
    assert (mates.n, mates.n % 16, mates.actors, np.unique(mates.who).size) == (3381, 5, 112, 110)
    assert [mates.family(f[0]) for f in fams] == [(0, 1440), (1440, 1536), (2976, 160), (3136, 245)]
    for t0 in MQ.T0S:
        states, moves = mates.distinct(t0)
        assert all(EQ.uploadable(s) for s in states), t0
        q = mates.at(t0)
        assert q.placed.tobytes() == states[mates.who].tobytes() and np.array_equal(q.placed_moves, mates.script[t0])
        assert all(q.order[q.env_of(j, r)] == j for j in q.held for r in range(3)) and q.held.size == 110
    assert mates.at(0).placed.tobytes() == mates.start.tobytes()
    # the state at t0 = 1 is the solo trace after tick 0, and the first tick played on it is the trace's tick 1
    s, mv = (a.copy() for a in mates.distinct(1))
    for j in (0, 17, 60, 93, 111):
        mates.oracle.step(s[j:j + 1], mv[j])
    s["agents"]["pad"] = 0
    assert all(s[j].tobytes() == mates.stage.states[j, 1].tobytes() for j in (0, 17, 60, 93, 111))


def test_queries_with_an_order_of_their_own_reuse_the_per_state_checkers(mates):
    """order = the composition: the per-state answers are gathered by it; jobs() and expand() name an env of every state the order holds"""
    q = mates.at(0)
    assert q.n == mates.n and q.d == 112 and np.array_equal(q.order, mates.who)
    flame, agent, ub = q.forecast(True)
    assert flame.shape[0] == agent.shape[0] == 112 and flame[q.order].shape[0] == mates.n
    src, mv, words = q.jobs()
    assert len(src) == 110 + 22 and set(q.order[src].tolist()) == set(q.held.tolist()) and words.shape == (EQ.ROLLOUT_R, len(src))
    src, want, status, words = q.expand(0)
    assert np.array_equal(q.order[src], q.held) and want.size == mates.n + 110 and want[:mates.n].tobytes() == q.placed.tobytes()
    h = mates.once_each(0)
    assert h.n == 112 and np.array_equal(h.held, np.arange(112)) and [h.env_of(j, 2) for j in (0, 5, 111)] == [0, 5, 111]


@pytest.mark.parametrize("mask", MQ.MASKS, ids=["mask_0110", "mask_1111"])
def test_simple_agents_do_not_disarm_the_actors(mates, mask):
    states = mates.played(mask)[0]
    kinds = np.array(mates.stage.cast.kinds)[mates.who]
    assert {k: len({int(a) for a in mates.who[kinds == k]}) for k in ("deep_b", "deep_top", "select", "claims_full")} == \
        {"deep_b": 18, "deep_top": 12, "select": 61, "claims_full": 1}   # (select_idx13 / _idx19 sit in no composition: 63 - 2)
    for t in range(4):
        g = np.ascontiguousarray(states[t]).reshape(-1).view(STATE_DTYPE)
        w = np.ascontiguousarray(mates.stage.states[mates.who, t]).reshape(-1).view(STATE_DTYPE)
        same = np.ones(mates.n, bool)
        for f in ("bombs_queue", "bombs_index", "bombs_count", "flames_count"):
            same &= (g[f].reshape(mates.n, -1) == w[f].reshape(mates.n, -1)).all(axis=1)
        for k in ("deep_b", "deep_top", "select"):
            assert same[kinds == k].all(), (k, t, mates.name_of_env(np.nonzero((kinds == k) & ~same)[0][0]))
        if t == 0:
            assert same[kinds == "claims_full"].all() and int((kinds == "claims_full").sum()) == 412
        if t == 1:
            assert int(same[kinds == "claims_full"].sum()) == 335
        assert len({int(a) for a in mates.who[(kinds == "bounce") & ~same]}) == 6   # the scripts are what exercises them: mask 0


def test_no_env_raises_a_fatal_flag_under_any_mask(mates):
    """16 ticks, the scripts and both SimpleAgent masks: LOST_AGENT only — the GPU module exempts nothing"""
    for mask in (0,) + MQ.MASKS:
        ub = mates.played(mask)[1]
        flags = int(np.bitwise_or.reduce(ub.ravel()))
        assert not flags & (FATAL | UB_FLAME_QUEUE_RANGE) and flags == (0 if mask == 0xF else 1), (mask, hex(flags))
    # mask 0 through the model is the solo traces: the first GPU test may compare against either
    states, ub, _, _ = mates.played(0)
    one_alive = mates.who == mates.stage.cast.ix["quiet_one_alive"]   # (MODE_ENV: done after its first tick, then not stepped)
    for t in (0, 1, 15):
        w = mates.stage.states[mates.who, t].copy().reshape(-1).view(STATE_DTYPE)
        g = np.ascontiguousarray(states[t]).reshape(-1).view(STATE_DTYPE)
        rest = ~one_alive & ~(g["aliveAgents"] <= 1)
        assert (g["board"][rest] == w["board"][rest]).all() and np.array_equal(ub[t][rest], mates.stage.sticky[mates.who, t][rest])


@pytest.mark.parametrize("mask", (0,) + MQ.MASKS, ids=["scripts", "mask_0110", "mask_1111"])
def test_restart_family_restarts_beside_detonating_mates(mates, mask):
    """cap ENV_CAP, 3 cap + 2 ticks: every env restarts at least twice; wavefronts in which 0, 1, 2, 15 and 16 envs restart on one
    tick occur in all three modes; the counts are the model's (the same under every mask: a game here ends by the cap)"""
    ticks = 3 * TM.ENV_CAP + 2
    for mode, (steps, episodes, resets) in (((RESET_AT_START, False), (3200, 1459, 1400)), ((RESET_AT_START, True), (3200, 539, 536)),
                                            ((RESET_AT_END, False), (3200, 1459, 1459))):
        frames = mates.restarts(mode, mask)
        assert len(frames) == ticks
        r = frames[-1][0].readable()
        assert r["counters"][:3].tolist() == [steps, episodes, resets], (mode, r["counters"].tolist())
        per_env = np.bincount(np.concatenate([np.array(f[1], dtype=np.int64) for f in frames]), minlength=160)
        assert per_env.min() >= 2, mode
        per_wave = {sum(1 for e in f[1] if e // 16 == w) for f in frames for w in range(10)}
        assert {0, 1, 2, 15, 16} <= per_wave, (mode, sorted(per_wave))
        if mask and mode[0] == RESET_AT_START:   # a restart wipes a memory that held something
            wiped = 0
            for (_, restarted), (before, _) in zip(frames[1:], frames):
                wiped += int(before.readable()["memory"][list(restarted)].any(axis=(1, 2)).sum())
            assert wiped > 100, wiped


def test_the_search_calls_have_something_to_say_on_the_batch(mates):
    for t0 in MQ.T0S:
        q = mates.at(t0)
        flame, agent, ub = q.forecast(True)
        assert (flame[q.order] > 0).any() and (agent > 0).any() and (agent == 0).any()
        for h in EQ.FORECAST_PREFIXES:
            assert int(q.forecast(True, h)[0].max()) <= h
        death, escape = q.move_safety(False)
        assert (death > 0).any() and (death == 0).any()
        mems, moves = mates.memory(t0)
        assert int(mems.any(axis=(1, 2)).sum()) > 3000 and (moves != 0).any()   # the parked dwords are not zero
        kept, fresh = mates.rollout_policy(t0, False), mates.rollout_policy(t0, True)
        assert (kept != fresh).any() and kept.shape == (MQ.POLICY_R, mates.n)
        src, mv, words = mates.jobs(t0)
        assert (len(src), len(src) % 16, int((src < 0).sum())) == (3381 + 11 + 112, 0, 11) and not words[:, src < 0].any()
        assert np.array_equal(src[:mates.n], mates.who) and np.array_equal(src[-112:], np.arange(112)) and (words[:, src >= 0] != 0).all()
    for mode in (0, 1):
        (src0, _, both0, st0, w0), (src1, _, both1, st1, w1) = mates.expand(mode)
        assert np.array_equal(src0, mates.who) and np.array_equal(src1, np.arange(112, 112 + mates.n))
        assert both0[:112].tobytes() == both1[:112].tobytes() == mates.distinct(0)[0].tobytes()
        assert ((w0 >> 16) == 1).all() and ((w1 >> 16) == 1).sum() > 3000
        if mode == 0:   # RAW: the children are the solo traces at ticks 0 and 1
            for t, both in ((0, both0), (1, both1)):
                assert both[112:].tobytes() == mates.stage.states[mates.who, t].tobytes()
