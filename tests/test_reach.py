"""pom_batch_reach on the GPU (include/pom_batch.h PomReachSpec): every agent's FillRMap distances and first moves in one launch, byte for
byte the compiled reference's (tests/golden/reach.npz) and the oracle's restatement on played boards; the mask, either output alone,
max_dist, tile mates and launch shapes change nothing they should not; the batch is left exactly as it was; bad arguments are refused
by name.  What the call has to say is known before the GPU runs."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import reach_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reach.npz")
MAX_DISTS = (1, 2, 10, 63, 64, 120)
SENTINEL = 0xAA   # no distance (<= 120) and no Move (<= 4) is 170
PAD = 7           # the fixture's 452 States and 7 more: 28 whole tiles and a last one of 11


@functools.lru_cache(maxsize=None)
def _fixture():
    """(states with the padding, dist, move) — computed once and shared, nobody writes to them"""
    g = np.load(GOLDEN)
    ix = np.concatenate([np.arange(len(g["names"])), np.arange(PAD)])
    states = g["states"][ix].copy().view(STATE_DTYPE).reshape(-1)
    assert states.size % 16 != 0 and states.size > 16 * 16
    dist, move = RC.expected_planes(states, g["map121"][ix], g["move_to121"][ix])
    for a in (states, dist, move):
        a.setflags(write=False)
    return states, dist, move


def _cut(dist, move, max_dist):
    """the full result with the cells farther than max_dist zeroed, in both planes"""
    far = dist > max_dist
    return np.where(far, 0, dist), np.where(far, 0, move)


def _env(states, **kw):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    kw.setdefault("mode", MODE_ENV)
    env = BatchEnvironment(len(states), **kw)
    env.make_game(states)
    return env


def _same(got, want, what):
    for name, w in zip(("dist", "move"), want):
        if name not in got:
            continue
        g = got[name].cpu().numpy()
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {name} differs in {len(bad)} places, first (env, agent, y, x) {bad[0].tolist()}: got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"


@pytest.mark.gpu
def test_fixture_parity(hip_lib):
    """the fixture's States in a handle whose size is no multiple of 16: all four agents' planes as the compiled reference gave them;
    dead agents' rows are zero"""
    import torch
    states, dist, move = _fixture()
    with _env(states) as env:
        got = env.reach()
        assert set(got) == {"dist", "move"} and all(t.dtype == torch.uint8 and tuple(t.shape) == (states.size, 4, 11, 11) for t in got.values())
        _same(got, (dist, move), "fixture")
        dead = torch.from_numpy(states["agents"]["dead"] != 0).to("cuda")
        assert int(dead.sum()) > 100 and not got["dist"][dead].any() and not got["move"][dead].any()
        assert int(got["dist"].max()) == 70


@pytest.mark.gpu
def test_rows_outside_the_mask_are_not_written(hip_lib):
    """every mask 1..15, the outputs inside larger buffers of 0xAA: the rows of the agents not asked for, and the bytes around the
    outputs, keep it"""
    import torch
    states, dist, move = _fixture()
    n = states.size
    with _env(states) as env:
        for mask in range(1, 16):
            bufs = [torch.full((8 + n * 484 + 64,), SENTINEL, dtype=torch.uint8, device="cuda") for _ in range(2)]
            assert all(b.data_ptr() % 8 == 0 for b in bufs)
            out = {name: b[8:8 + n * 484].view(n, 4, 11, 11) for name, b in zip(("dist", "move"), bufs)}
            got = env.reach(agents=mask, out=out)
            assert got["dist"].data_ptr() == out["dist"].data_ptr() and got["move"].data_ptr() == out["move"].data_ptr()
            rows = [a for a in range(4) if mask >> a & 1]
            others = [a for a in range(4) if not mask >> a & 1]
            _same({k: v[:, rows] for k, v in got.items()}, (dist[:, rows], move[:, rows]), f"mask {mask:#x}")
            for b in bufs:
                assert (b[:8] == SENTINEL).all() and (b[8 + n * 484:] == SENTINEL).all(), mask
            for t in got.values():
                assert (t[:, others] == SENTINEL).all(), mask
        # a tensor the call allocates: the rows not asked for are 0
        got = env.reach(agents=[1, 2])
        assert not got["dist"][:, [0, 3]].any() and not got["move"][:, [0, 3]].any()
        _same({k: v[:, [1, 2]] for k, v in got.items()}, (dist[:, [1, 2]], move[:, [1, 2]]), "agents [1, 2]")


@pytest.mark.gpu
def test_one_output_alone_gives_the_same_bytes(hip_lib):
    states, dist, move = _fixture()
    with _env(states) as env:
        for max_dist in (120, 10):
            want = _cut(dist, move, max_dist)
            d = env.reach(max_dist=max_dist, move=False)
            m = env.reach(max_dist=max_dist, dist=False)
            assert set(d) == {"dist"} and set(m) == {"move"}
            _same(d, want, f"dist alone, max_dist {max_dist}")
            _same(m, want, f"move alone, max_dist {max_dist}")


@pytest.mark.gpu
@pytest.mark.parametrize("max_dist", MAX_DISTS)
def test_max_dist_zeroes_the_farther_cells(hip_lib, max_dist):
    states, dist, move = _fixture()
    want = _cut(dist, move, max_dist)
    assert max_dist >= 64 or (want[0] != dist).any()
    with _env(states) as env:
        _same(env.reach(max_dist=max_dist), want, f"max_dist {max_dist}")


@pytest.mark.gpu
def test_rows_do_not_depend_on_the_tile_mates(hip_lib):
    """the envs of every tile permuted — each env among other mates and in another column of its wavefront, the long floods beside
    the short ones: its rows are the same"""
    states, dist, move = _fixture()
    n = states.size
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)                                      # any env into any tile and column
    with _env(states[perm].copy()) as env:
        _same(env.reach(), (dist[perm], move[perm]), "shuffled over the batch")
    inside = np.concatenate([t + rng.permutation(min(16, n - t)) for t in range(0, n, 16)])   # the same mates, other columns
    assert (inside // 16 == np.arange(n) // 16).all() and (inside != np.arange(n)).sum() > n // 2
    with _env(states[inside].copy()) as env:
        _same(env.reach(), (dist[inside], move[inside]), "shuffled inside the tiles")


def _everything(env, terminal=True):
    """all the API can read of a handle (the terminal records and last results: of a handle with end-of-tick resets only)"""
    out = dict(state=env.get_state().tobytes(), counters=env.counters().tolist(), episodes=env.episodes().tolist(),
               memory=env.policy_memory().tobytes(), chain=env.chain_stats())
    out.update({"status_" + k: v.tolist() for k, v in env.status().items()})
    if terminal:
        out["terminal"] = env.get_terminal_state().tobytes()
        out.update({"last_" + k: v.tolist() for k, v in env.last_results().items()})
    return out


@pytest.mark.gpu
def test_reach_leaves_no_trace(hip_lib):
    """an ENV-mode handle with end-of-tick resets and fresh boards, in the middle of SimpleAgent games: everything the API can read is
    the same before and after the calls, and 20 more ticks equal a twin's that never asked"""
    from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
    n, kw = 200, dict(mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    with BatchEnvironment(n, **kw) as env, BatchEnvironment(n, **kw) as twin:
        for e in (env, twin):
            e.generate(9)
            e.step_simple(3, 40)
        before = _everything(env)
        assert _everything(twin) == before
        assert sum(before["last_finished"]) + sum(before["episodes"]) > 0 and before["counters"][0] == n * 40
        for kwargs in (dict(), dict(agents=[1], max_dist=5), dict(agents=0xA, move=False), dict(dist=False)):
            got = env.reach(**kwargs)
            assert all(int(t.sum()) > 0 for t in got.values())
            assert _everything(env) == before, kwargs
        env.step_simple(3, 20)
        env.reach()
        twin.step_simple(3, 20)
        assert _everything(env) == _everything(twin)


@pytest.mark.gpu
def test_reach_after_chained_launches_settles(hip_lib, oracle):
    """20 chained ticks, then the call with nothing in between: the maps are those of the state a download returns, no launch is
    added to the chain, and a twin that never asked reads the same afterwards"""
    from pomcpp_amd.batch import DIST_RANDOM, ISSUE_CHAIN, MODE_ENV
    from tests import forecast_cases as FC
    n = 600
    start = FC.played_states(oracle, "stress", n, 23)
    kw = dict(mode=MODE_ENV, auto_reset=True, max_steps=300, issue_mode=ISSUE_CHAIN)
    with _env(start, **kw) as env, _env(start, **kw) as twin:
        assert env.issue_info()[0] == "chain"
        for e in (env, twin):
            e.step_random(5, DIST_RANDOM, ticks=20)
        got = env.reach()
        assert env.chain_stats()["launches"] == 20
        now = env.get_state()
        _same(got, RC.expected_planes(now, *RC.fill_rmap(oracle, now)), "after 20 chained ticks")
        mine, theirs = _everything(env, terminal=False), _everything(twin, terminal=False)
        assert mine.pop("chain")["launches"] == theirs.pop("chain")["launches"] == 20   # (its other numbers depend on timing)
        assert mine == theirs


@pytest.mark.gpu
@pytest.mark.parametrize("epw,lpe", [(16, 4), (16, 1), (32, 1), (64, 1)])
def test_handle_shapes_give_the_same_bytes(hip_lib, epw, lpe):
    """the call's own launch shape does not depend on the handle's: the device buffers are 16-env tiles whatever the shape"""
    states, dist, move = _fixture()
    with _env(states, envs_per_wave=epw, lanes_per_env=lpe) as env:
        assert env.launch_shape()[:2] == (epw, lpe)
        _same(env.reach(), (dist, move), f"epw {epw} lanes {lpe}")


@pytest.mark.gpu
def test_mid_game_parity_with_the_oracle(hip_lib, oracle):
    """1,040 envs played 40 ticks by SimpleAgent on the device: the planes equal the oracle's FillRMap on the downloaded States, for
    all agents — bombs, flames, power-ups and dead agents among them"""
    from pomcpp_amd.batch import MODE_ENV, BatchEnvironment
    n = 1040
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800, fresh_boards=True, board_seed=21) as env:
        env.generate(21)
        env.step_simple(5, 40)
        got = env.reach()
        now = env.get_state()
    want = RC.expected_planes(now, *RC.fill_rmap(oracle, now))
    board = now["board"]
    assert (board == 3).any() and ((board >> 16) == 4).any() and ((board >= 6) & (board <= 8)).any() and (now["agents"]["dead"] != 0).any()
    assert want[0].max() >= 20
    _same(got, want, "after 40 SimpleAgent ticks")


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """every POM_E_ARG case of the header, with the call's name in the message, and nothing written"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _ReachSpec
    states = _fixture()[0][:32].copy()
    n = states.size
    with _env(states) as env:
        lib, h = env._lib, env._h
        dbuf = torch.full((n * 484 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        mbuf = torch.full((n * 484 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        size, d, m = C.sizeof(_ReachSpec), dbuf.data_ptr(), mbuf.data_ptr()
        bad = {
            "struct_size": _ReachSpec(size - 8, 15, 120, 0, d, m, 0),
            "agent_mask 0": _ReachSpec(size, 0, 120, 0, d, m, 0),
            "agent_mask 16": _ReachSpec(size, 16, 120, 0, d, m, 0),
            "agent_mask -1": _ReachSpec(size, -1, 120, 0, d, m, 0),
            "max_dist 0": _ReachSpec(size, 15, 0, 0, d, m, 0),
            "max_dist 121": _ReachSpec(size, 15, 121, 0, d, m, 0),
            "reserved_": _ReachSpec(size, 15, 120, 1, d, m, 0),
            "reserved2_": _ReachSpec(size, 15, 120, 0, d, m, 1),
            "both outputs null": _ReachSpec(size, 15, 120, 0, None, None, 0),
            "dist + 4": _ReachSpec(size, 15, 120, 0, d + 4, m, 0),
            "move + 1": _ReachSpec(size, 15, 120, 0, None, m + 1, 0),
        }
        before = env.get_state().tobytes()
        for what, spec in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_reach(h, C.byref(spec)))
            assert err.value.code == 1 and "pom_batch_reach" in str(err.value), what
        good = _ReachSpec(size, 15, 120, 0, d, m, 0)
        for call in (lambda: lib.pom_batch_reach(None, C.byref(good)), lambda: lib.pom_batch_reach(h, None)):
            with pytest.raises(PomError) as err:
                _check(lib, call())
            assert err.value.code == 1 and "pom_batch_reach" in str(err.value)
        env.sync()
        assert (dbuf == SENTINEL).all() and (mbuf == SENTINEL).all()
        assert env.get_state().tobytes() == before
        for kw in (dict(max_dist=0), dict(max_dist=121), dict(agents=16), dict(agents=[4]), dict(agents=[]), dict(dist=False, move=False),
                   dict(out={"dist": dbuf[:n * 484].view(n, 4, 121)}), dict(out={"move": mbuf[:n * 484].view(n, 4, 11, 11).to(torch.int8)})):
            with pytest.raises(ValueError):
                env.reach(**kw)
        # the outputs need 8-byte alignment only: a call 8 bytes into the buffers runs
        _check(lib, lib.pom_batch_reach(h, C.byref(_ReachSpec(size, 15, 120, 0, d + 8, m + 8, 0))))
        env.sync()
        assert not (dbuf[8:8 + n * 484] == SENTINEL).any() and not (mbuf[8:8 + n * 484] == SENTINEL).any()
        assert (dbuf[:8] == SENTINEL).all() and (dbuf[8 + n * 484:] == SENTINEL).all() and (mbuf[8 + n * 484:] == SENTINEL).all()
