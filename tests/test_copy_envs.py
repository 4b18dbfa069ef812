"""GPU: copy and restore games by index (pom_batch_copy_envs / _copy_envs_device, BatchEnvironment.copy_envs / restore) — bit-exact
against downloaded states and the oracle (tests/oracle_lib.py)."""
import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import (BatchEnvironment, MODE_ENV, DIST_RANDOM, DIST_STRESS, RESET_AT_END, RESET_AT_START, RESET_OFF,
                              ISSUE_CHAIN, CNT_STEPS, PomError)

pytestmark = pytest.mark.gpu


def _bytes(s):
    s = s.copy()
    s["agents"]["pad"] = 0
    return s.view(np.uint8).reshape(s.size, -1)


def _same(got, want):
    return np.array_equal(_bytes(got), _bytes(want))


def _midgame(n, seed, ticks=30, kind="stress"):
    """n states some 30 ticks into games that are still running (two or more agents alive): live bombs, flames, kicked bombs"""
    m = 3 * n
    start = pa.make_boards(m, seed=seed, kind=kind)
    with BatchEnvironment(m, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(start)
        env.step_random(seed, DIST_STRESS, ticks=ticks)
        out = env.get_state()
    out = np.ascontiguousarray(out[out["aliveAgents"] > 1][:n])
    assert out.size == n and (out["bombs_count"] > 0).mean() > 0.5 and (out["flames_count"] > 0).mean() > 0.2
    return out


@pytest.fixture(scope="module")
def roots():
    return _midgame(1000, seed=41)


@pytest.mark.parametrize("first,count", [(5, 23), (600, 23), (0, 1000)])
def test_fan_out_unaligned(hip_lib, roots, first, count):
    """src = i % R over a range that is not tile-aligned, n = 1000 (not a multiple of 16); first = 5 has sources inside the range
    (the scratch pass), first = 600 does not (the host variant's one-pass shortcut)"""
    n, R = 1000, 7
    src = np.arange(count, dtype=np.int64) % R
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(roots)
        env.step_simple(3, 2)  # agent memory and a tick of their own for every env
        before, mem, eps = env.get_state(), env.policy_memory(), env.episodes()
        env.copy_envs(src, first)
        after, mem2, eps2 = env.get_state(), env.policy_memory(), env.episodes()
    want = before.copy()
    want[first:first + count] = before[src]
    assert _same(after, want)
    wmem = mem.copy()
    wmem[first:first + count] = mem[src]
    assert np.array_equal(mem2, wmem) and mem[:R].any()
    weps = eps.copy()
    weps[first:first + count] = eps[src]
    assert np.array_equal(eps2, weps)


def test_in_place_permutation_with_repeats_host_and_device(hip_lib, roots):
    import torch
    n = 1000
    rng = np.random.default_rng(8)
    src = rng.integers(0, n, n).astype(np.int64)  # a resample with repeats over the whole batch
    outs = []
    for variant in ("host", "device"):
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
            env.make_game(roots)
            before = env.get_state()
            env.copy_envs(torch.from_numpy(src).to(f"cuda:{env.device}") if variant == "device" else src)
            got = env.get_state()
            assert _same(got, before[src]), variant
            outs.append(got)
    assert _same(outs[0], outs[1])


def test_one_pass_shortcut_equals_scratch_path(hip_lib, roots):
    """no source in the destination range: the host variant writes in one pass, the device variant always through the scratch;
    states, agent memory, episodes and (set_snapshot) snapshots come out the same"""
    import torch
    n, first, count = 1000, 500, 400
    src = np.random.default_rng(9).integers(0, first, count).astype(np.int64)
    src[::17] = -1
    res = []
    for variant in ("host", "device"):
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
            env.make_game(roots)
            env.step_simple(4, 3)
            idx = torch.from_numpy(src).cuda(env.device) if variant == "device" else src
            env.copy_envs(idx, first, set_snapshot=True)
            st, mem, eps = env.get_state(), env.policy_memory(), env.episodes()
            env.restore(np.ones(n, dtype=bool))
            res.append((st, mem, eps, env.get_state()))
    (a, am, ae, asnap), (b, bm, be, bsnap) = res
    assert _same(a, b) and np.array_equal(am, bm) and np.array_equal(ae, be) and _same(asnap, bsnap)
    keep = np.arange(first, first + count)[src < 0]
    assert _same(asnap[keep], roots[keep])  # masked entries kept their own snapshot


@pytest.mark.parametrize("chain", [False, True])
def test_clones_continue_like_the_oracle_under_step_random(hip_lib, oracle, roots, chain):
    """K ticks, a resample, K more: equals the oracle on the gathered states, keyed by the DESTINATION env indices; with chained
    launches on both sides of the copy (and no tile left behind)"""
    n, cap, seed, K = 1000, 800, 12, 12
    src = np.random.default_rng(10).integers(0, n, n).astype(np.int64)
    kw = dict(issue_mode=ISSUE_CHAIN) if chain else {}
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=cap, **kw) as env:
        env.make_game(roots)
        env.step_random(seed, DIST_RANDOM, ticks=K)
        env.copy_envs(src)
        env.step_random(seed, DIST_RANDOM, ticks=K)
        got = env.get_state()
        if chain:
            assert env.chain_stats()["tiles_recovered"] == 0 and env.issue_info()[0] == "chain"
        assert env.counters()[CNT_STEPS] == 2 * K * n
    ref = roots.copy()
    oracle.run_random(ref, roots, K, seed, 0, 0, DIST_RANDOM, cap)
    ref = np.ascontiguousarray(ref[src])
    oracle.run_random(ref, roots, K, seed, 0, K, DIST_RANDOM, cap)  # the snapshot stays the destination's own
    assert _same(got, ref)
    assert len(np.unique(_bytes(got)[np.flatnonzero(src == src[0])], axis=0)) > 1 or np.count_nonzero(src == src[0]) == 1


def test_simple_agent_memory_travels_with_the_game(hip_lib, oracle, roots):
    n, cap, seed = 512, 800, 21
    start = np.ascontiguousarray(roots[:n])
    src = np.random.default_rng(11).integers(0, n, n).astype(np.int64)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=cap) as env:
        env.make_game(start)
        env.step_simple(seed, 10)
        mem_before = env.policy_memory()
        env.copy_envs(src)
        assert np.array_equal(env.policy_memory(), mem_before[src])
        env.step_simple(seed, 10)
        got, mem = env.get_state(), env.policy_memory()
    ref, mems = start.copy(), np.zeros((n, 4, 16), dtype=np.int32)
    oracle.run_simple(ref, start, mems, 10, seed, 0, 0, cap)
    assert np.array_equal(mems, mem_before)
    ref, mems = np.ascontiguousarray(ref[src]), np.ascontiguousarray(mems[src])
    oracle.run_simple(ref, start, mems, 10, seed, 0, 10, cap)
    assert _same(got, ref) and np.array_equal(mem, mems)


def test_restore_mask_and_list(hip_lib, roots):
    n = 1000
    rng = np.random.default_rng(12)
    mask = rng.random(n) < 0.05
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(roots)
        env.step_simple(5, 6)
        before, mem, eps = env.get_state(), env.policy_memory(), env.episodes()
        env.restore(mask)
        got, mem2 = env.get_state(), env.policy_memory()
        assert _same(got[mask], roots[mask]) and _same(got[~mask], before[~mask])
        assert not mem2[mask].any() and np.array_equal(mem2[~mask], mem[~mask]) and mem[mask].any()
        assert np.array_equal(env.episodes(), eps)
        env.restore([999, 3, 3, 640])
        got2 = env.get_state()
        picked = np.zeros(n, dtype=bool)
        picked[[3, 640, 999]] = True
        assert _same(got2[picked], roots[picked]) and _same(got2[~picked], got[~picked])


def test_set_snapshot_clone_restarts_on_its_root(hip_lib, oracle, roots):
    """POM_RESET_AT_START: a clone made with set_snapshot restarts on the root it was cloned from, not on its own old start"""
    n, seed = 64, 31
    start = np.ascontiguousarray(roots[100:100 + n])
    cap = int(start["timeStep"][0]) + 25
    src = np.zeros(n - 1, dtype=np.int64)  # root = env 0, fanned out over envs 1..63
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_START, max_steps=cap) as env:
        env.make_game(start)
        env.copy_envs(src, 1, set_snapshot=True)
        env.step_random(seed, DIST_RANDOM, ticks=60)
        got = env.get_state()
    init = np.ascontiguousarray(np.repeat(start[:1], n))
    ref = init.copy()
    oracle.run_random(ref, init, 60, seed, 0, 0, DIST_RANDOM, cap)
    assert _same(got, ref)
    assert (got["timeStep"] < int(start["timeStep"][0]) + 60).all()  # every clone has restarted (on the root: the oracle's init)
    assert len(np.unique(_bytes(got), axis=0)) > 1  # the clones diverged: their env index keys their moves


def test_at_end_results_terminal_and_fresh_board_episodes(hip_lib, oracle):
    """POM_RESET_AT_END with fresh boards: last results, terminal state and episode counter are copied; a clone's next board is
    the one of (destination env, copied episode + 1)"""
    n, cap, bseed, seed = 256, 20, 77, 5
    src = np.random.default_rng(13).integers(0, n, n).astype(np.int64)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=cap, fresh_boards=True, board_seed=bseed) as env:
        env.generate(bseed)
        env.step_random(seed, DIST_RANDOM, ticks=47)
        lr, term, eps, st = env.last_results(), env.get_terminal_state(), env.episodes(), env.get_state()
        assert (lr["length"] > 0).all() and (eps > 0).all()  # every env has finished an episode
        env.copy_envs(src)
        lr2 = env.last_results()
        for k in lr:
            assert np.array_equal(lr2[k], lr[k][src]), k
        assert _same(env.get_terminal_state(), term[src]) and _same(env.get_state(), st[src])
        ep2 = env.episodes()
        assert np.array_equal(ep2, eps[src])
        seen = np.zeros(n, dtype=bool)
        for _ in range(cap + 1):
            env.step_random(seed, DIST_RANDOM, ticks=1)
            fin = env.last_results()["finished"].astype(bool) & ~seen
            if fin.any():
                e = np.flatnonzero(fin)
                assert np.array_equal(env.episodes()[e], ep2[e] + 1)
                assert _same(env.get_state()[e], oracle.boardgen(bseed, e, ep2[e] + 1))
                seen |= fin
        assert seen.all()


def test_device_indices_in_stream_order_with_out_of_range_entries(hip_lib, roots):
    import torch
    n = 1000
    rng = np.random.default_rng(14)
    src = rng.integers(0, n, n).astype(np.int64)
    src[rng.random(n) < 0.1] = -1
    big = rng.random(n) < 0.1
    raw = src.copy()
    raw[big] = n + rng.integers(0, 1 << 40, int(big.sum()))
    host = np.where(big, -1, src)
    dev = torch.device("cuda", 0)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as a, \
         BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as b:
        a.make_game(roots)
        b.make_game(roots)
        before = a.get_state()
        a.copy_envs(host)
        staged = torch.from_numpy(raw).to(dev)
        idx = torch.full((n,), 7, dtype=torch.int64, device=dev)
        torch.cuda.synchronize(dev)
        torch.cuda._sleep(2_000_000)  # keep torch's current stream busy: the copy must wait for the write queued behind it
        idx.copy_(staged)
        b.copy_envs(idx)
        ga, gb = a.get_state(), b.get_state()
    assert _same(ga, gb)
    keep = host < 0
    assert _same(gb[keep], before[keep]) and _same(gb[~keep], before[host[~keep]])


def test_host_variant_rejects_bad_arguments_and_changes_nothing(hip_lib, roots):
    from pomcpp_amd.batch import _check
    n = 100
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(roots[:n])
        before = env.get_state()
        for src, first, flags in (([1, 2, n], 0, 0), ([1, 2, n + 5, 3], 10, 0), ([1, 2], -1, 0), ([1, 2], n - 1, 0), ([1, 2], 0, 4)):
            idx = np.asarray(src, dtype=np.int64)
            with pytest.raises(PomError) as e:
                _check(env._lib, env._lib.pom_batch_copy_envs(env._h, idx.ctypes.data, first, idx.size, flags))
            assert e.value.code == 1, (src, first, flags)
        with pytest.raises(PomError):
            env.copy_envs(np.asarray([0, n]), 10)
        assert _same(env.get_state(), before)


def test_observation_of_a_clone_equals_its_source(hip_lib, roots):
    n = 1000
    src = np.random.default_rng(15).integers(0, n, n).astype(np.int64)
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
        env.make_game(roots)
        p0, a0, e0 = (t.cpu().numpy() for t in env.observe(attrs=True))
        env.copy_envs(src)
        p1, a1, e1 = (t.cpu().numpy() for t in env.observe(attrs=True))
    assert np.array_equal(p1, p0[src]) and np.array_equal(a1, a0[src]) and np.array_equal(e1, e0[src])


def _outcome(states):
    """per env, for agent 0: 1 win (the last one alive), -1 loss (dead), 0 otherwise (draw or undecided)"""
    dead0 = states["agents"]["dead"][:, 0] != 0
    return np.where(dead0, -1, np.where(states["aliveAgents"] == 1, 1, 0))


def test_flat_monte_carlo_evaluation_matches_the_oracle(hip_lib, oracle, roots):
    """R roots x 6 first moves of agent 0 x M rollouts of K ticks: fan-out, one step with the candidate move, step_random; win /
    draw / loss counts per (root, move) equal the oracle's for the same env indices and seed"""
    R, M, K, seed = 4, 16, 40, 99
    root = np.ascontiguousarray(roots[200:200 + R])
    n = R + R * 6 * M
    src = np.repeat(np.arange(R), 6 * M).astype(np.int64)
    first_move = np.tile(np.repeat(np.arange(6), M), R)
    rng = np.random.default_rng(16)
    moves = rng.integers(0, 6, (n, 4)).astype(np.int32)
    moves[R:, 0] = first_move
    with BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_OFF) as env:
        batch = np.zeros(n, dtype=root.dtype)
        batch[:R] = root
        batch[R:] = root[0]
        env.make_game(batch)
        env.copy_envs(src, R)
        env.step(moves)
        env.set_tick(0)
        env.step_random(seed, DIST_RANDOM, ticks=K)
        got, st = env.get_state(), env.status()
    ref = np.ascontiguousarray(root[src])
    for i in range(ref.size):
        e = R + i
        one = ref[i:i + 1]
        status = dict(done=0, winner=-1, draw=0)
        if one["aliveAgents"][0] > 1:
            oracle.env_step(one, moves[e], status)
        for t in range(K):
            if one["aliveAgents"][0] <= 1:
                break
            oracle.run_random(one, one.copy(), 1, seed, e, t, DIST_RANDOM, 0)
        ref[i:i + 1] = one
    assert _same(got[R:], ref)
    want, have = _outcome(ref), _outcome(got[R:])
    assert np.array_equal(st["winner"][R:] == 0, want == 1)
    table_want = np.zeros((R, 6, 3), dtype=int)
    table_have = np.zeros((R, 6, 3), dtype=int)
    for i in range(ref.size):
        table_want[src[i], first_move[i], want[i] + 1] += 1
        table_have[src[i], first_move[i], have[i] + 1] += 1
    assert np.array_equal(table_have, table_want) and table_want.sum() == R * 6 * M
    assert (table_want[..., 0] > 0).any()  # some rollouts are decided within K ticks
