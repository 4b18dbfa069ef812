"""The search calls used the way a search uses them (include/pom_batch.h PomExpandSpec, PomRolloutJobsSpec): expand, evaluate the new
children with rollout_jobs, expand again from them — slots reused, a child of one round a source of the next, ordinary ticks in between
— against a host model of the handle (tests/search_model.py); and expand on a handle that chains its launches, with chained ticks on
both sides of it, against a handle that does not chain and against the checker.

The batch of the rounds is 72 envs: four whole tiles and a short one of 8, n_pad 128 (the buffers hold a multiple of 64 columns).  The rounds' lists are made once, from a seed, at
import; what they must contain is asserted at import too, so a change of the seed that loses a condition fails the collection."""
import numpy as np
import pytest

from tests import expand_oracle as XO
from tests import forecast_cases as FC
from tests import rollout_oracle as RO
from tests import search_model as SM
from tests.rollout_gpu import _dev, _env, _played, _words

N, N_PAD = 72, 128
RANGES = [(19, 18), (30, 27), (5, 21), (41, 30), (17, 29), (50, 19)]    # (first, count) of round r
STEP_ROUNDS = (1, 3)                                                    # the rounds that end with a tick of the whole batch
NEVER_WRITTEN = (0, 2)                                                  # where the two lineages begin: envs no range covers
LIST_SEED = 11
SEED = 99


def _make_rounds(seed):
    """per round (first, src int64 [count], moves int32 [count, 4]).  Every list holds: one source twice, an identity entry, a refused
    in-range foreign source, one of -1 / n / 2^40, a source out of a destination tile but outside the range where there is one, and the
    latest slot of two LINEAGES — lineage A begins in round 0 from env 0, lineage B in round 1 from env 2; each round's lineage entry
    names the slot the lineage's entry of the round before filled, so a game is handed on from round to round and reaches max_steps.
    The other entries are drawn from the envs outside the range, every other one from the slots earlier rounds filled."""
    rng = np.random.default_rng(seed)
    rounds, filled, lineage = [], [], {"A": NEVER_WRITTEN[0], "B": None}
    for r, (first, count) in enumerate(RANGES):
        if r == 1:
            lineage["B"] = NEVER_WRITTEN[1]
        inside = set(range(first, first + count))
        nxt = set(range(RANGES[r + 1][0], sum(RANGES[r + 1]))) if r + 1 < len(RANGES) else set()
        outside = np.array([e for e in range(N) if e not in inside])
        earlier = np.array([e for e in sorted(set(filled)) if e not in inside], dtype=np.int64)
        tiles = range(first // 16, (first + count - 1) // 16 + 1)
        near = np.array([e for t in tiles for e in range(16 * t, min(16 * t + 16, N)) if e not in inside])
        src = np.empty(count, dtype=np.int64)
        for j in range(count):
            src[j] = rng.choice(earlier) if earlier.size and j % 2 == 0 else rng.choice(outside)
        order = rng.permutation(count)
        # a lineage's slot must still stand when the next round reads it: not inside the next round's range
        free = [int(j) for j in order if first + int(j) not in nxt]
        rest = [int(j) for j in order if int(j) not in free[:2]]
        for name, j in zip(("A", "B"), free[:2]):
            if lineage[name] is not None:
                assert lineage[name] not in inside
                src[j] = lineage[name]
                lineage[name] = first + j
        twice, again, ident, refused, none, close = rest[:6]
        src[again] = src[twice]
        src[ident] = first + ident
        src[refused] = first + (refused + 1) % count
        src[none] = (-1, N, 1 << 40)[r % 3]
        if near.size:
            src[close] = rng.choice(near)
        moves = FC.random_moves(count, 100 * seed + r)
        if tuple(moves[twice]) == tuple(moves[again]):
            moves[again, 0] = (moves[again, 0] + 1) % 6
        job = np.array([XO.is_job(int(s), first + j, first, count, N) for j, s in enumerate(src)])
        filled += (first + np.nonzero(job)[0]).tolist()
        rounds.append((first, src, moves))
    return rounds


ROUNDS = _make_rounds(LIST_SEED)
STEP_MOVES = {r: FC.random_moves(N, 700 + r) for r in STEP_ROUNDS}


def _jobs(first, src):
    return np.array([XO.is_job(int(s), first + j, first, len(src), N) for j, s in enumerate(src)])


def _check_the_lists():
    assert len(ROUNDS) >= 5
    written, overlaps, close = set(), 0, 0
    for r, (first, src, moves) in enumerate(ROUNDS):
        count = len(src)
        assert first % 16 != 0 and (first + count) % 16 != 0 and first + count <= N, r
        job, dest = _jobs(first, src), first + np.arange(count)
        overlaps += bool(written & set(dest.tolist()))
        if r > 0:
            assert 3 * sum(int(s) in written for s in src[job]) >= int(job.sum()), (r, "a third of the jobs start from earlier children")
        tiles = {int(d) >> 4 for d in dest}
        close += any((int(s) >> 4) in tiles and not first <= s < first + count for s in src[job])
        # a repeated source with different move rows, an identity entry, a refused in-range foreign source, an entry outside the batch
        rows = {}
        for j in np.nonzero(job)[0]:
            rows.setdefault(int(src[j]), set()).add(tuple(moves[j]))
        assert any(len(v) > 1 for v in rows.values()), r
        assert (src == dest).any(), r
        assert ((src >= first) & (src < first + count) & (src != dest)).any(), r
        assert any(int(s) in (-1, N, 1 << 40) for s in src), r
        written |= set(dest[job].tolist())
    assert overlaps >= 2 and close >= 1
    assert not any(first <= e < first + len(src) for e in NEVER_WRITTEN for first, src, _ in ROUNDS)


_check_the_lists()


def _start(kind, ticks):
    """the played boards at one timeStep: the pool's games have restarted at various ticks, and the bound is timeStep + 6"""
    states = _played(kind, ticks)[:N].copy()
    states["timeStep"] = ticks
    return states


def test_the_model_is_the_checker(oracle):
    """two model rounds are two direct XO.expand calls, and the side arrays follow the copy rule on a list with a repeat, an identity
    entry, a refused entry and a -1: a copying job's destination has its source's entries as they were BEFORE the call, every other
    index keeps its own"""
    n, first = 40, 19
    states = _played("ffa", 57)[:n].copy()
    src = np.array([0, 5, 5, 22, 26, -1, 38, 17], dtype=np.int64)      # 22 is its own slot; 26 lies in the range and is not
    moves = FC.random_moves(len(src), 3)
    job = np.array([XO.is_job(int(s), first + j, first, len(src), n) for j, s in enumerate(src)])
    assert job.tolist() == [True, True, True, True, False, False, True, True]
    rng = np.random.default_rng(1)
    memory = rng.integers(1, 1 << 20, size=(n, 4, 16), dtype=np.int32)
    episodes = rng.integers(0, 9, size=n).astype(np.uint32)
    terminal = _played("stress", 23)[:n].copy()
    m = SM.SearchModel(oracle, states, XO.MODE_ENV, 60, memory=memory, episodes=episodes, terminal=terminal)
    want, status = states, None
    for rnd in range(2):
        before = m.memory.copy(), m.episodes.copy(), m.terminal.copy()
        want, status, want_words, ticks, newly = XO.expand(oracle, want, status, src, moves, first, XO.MODE_ENV, 60)
        c0 = list(m.counters)
        words = m.expand(src, moves, first)
        assert np.array_equal(words, want_words) and m.states.tobytes() == want.tobytes()
        assert all(np.array_equal(m.status[k], status[k]) for k in status)
        assert [a - b for a, b in zip(m.counters, c0)] == [ticks, newly, 0] and ticks == int(job.sum())
        copied = job & (src != first + np.arange(len(src)))
        D, S = first + np.nonzero(copied)[0], src[copied]
        keep = np.ones(n, dtype=bool)
        keep[D] = False
        for got, was in zip((m.memory, m.episodes, m.terminal), before):
            assert got[D].tobytes() == was[S].tobytes() and got[keep].tobytes() == was[keep].tobytes()
        assert (m.memory[first + 3] == before[0][first + 3]).all() and (m.memory[first + 1] == before[0][5]).all()
    # the tick of the whole batch is the expansion with the identity list
    mv = FC.random_moves(n, 4)
    want, status, want_words, ticks, newly = XO.expand(oracle, want, status, np.arange(n), mv, 0, XO.MODE_ENV, 60)
    mem = m.memory.copy()
    assert np.array_equal(m.step(mv), want_words) and m.states.tobytes() == want.tobytes() and np.array_equal(m.memory, mem)
    # ... and the playouts leave the model alone
    w = m.rollout_jobs(np.array([3, -1, 19]), 2, 1, SEED, simple=0xF)
    assert w.shape == (1, 3) and w[0, 0] and not w[0, 1] and m.states.tobytes() == want.tobytes() and np.array_equal(m.memory, mem)


def _run_model(m, on_round=None):
    """the rounds on the model alone -> the words of every round"""
    out = []
    for r, (first, src, moves) in enumerate(ROUNDS):
        out.append(m.expand(src, moves, first))
        if r in STEP_ROUNDS:
            m.step(STEP_MOVES[r])
    return out


def test_a_finished_child_becomes_a_source(oracle):
    """over the rounds in ENV mode with max_steps = timeStep + 6 at least one child comes back DONE, and a later round that names it as
    its source gets the unticked copy, length 0 — checked on the model, which runs without a GPU, so a change of the lists cannot
    lose it silently"""
    m = SM.SearchModel(oracle, _start("ffa", 57), XO.MODE_ENV, 57 + 6)
    words = _run_model(m)
    done_child, found, timed_out = set(), 0, 0
    for (first, src, _), w in zip(ROUNDS, words):
        job = _jobs(first, src)
        for j in np.nonzero(job)[0]:
            length, done = int(w[j]) >> XO.RO_LENGTH_SHIFT, bool(int(w[j]) & XO.RO_DONE)
            found += int(src[j]) in done_child and int(src[j]) != first + j and length == 0 and done
            timed_out += length == 1 and bool(int(w[j]) & XO.RO_TIMEOUT)
        for j in np.nonzero(job)[0]:
            (done_child.add if int(w[j]) & XO.RO_DONE else done_child.discard)(first + int(j))
    assert found >= 1 and timed_out >= 1


PARAMS = [("ffa", 57, False), ("stress", 23, False), ("ffa", 57, True), ("simple", 40, False)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,ticks,raw", PARAMS)
def test_search_rounds_match_the_model(hip_lib, oracle, kind, ticks, raw):
    """six rounds of expand / rollout_jobs over the new children / (rounds 1 and 3) a step_device tick of the whole batch: after every
    call the words and everything the API reads of the handle are the model's, and the playouts change nothing.  `simple`: fresh
    boards 40 ticks into SimpleAgent games, so the agents' memory is not zero and travels with the games"""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW, RESET_OFF
    mode, max_steps = (MODE_RAW if raw else MODE_ENV), ticks + 6
    states = pa.make_boards(N, seed=21) if kind == "simple" else _start(kind, ticks)
    with _env(states, mode=mode, auto_reset=RESET_OFF, max_steps=max_steps) as env:
        assert env.device_view()[1] == N_PAD
        if kind == "simple":
            env.step_simple(3, ticks)
        m = SM.SearchModel.of_handle(oracle, env, mode, max_steps)
        assert m.memory.any() == (kind == "simple")
        for r, (first, src, moves) in enumerate(ROUNDS):
            what = f"{kind} raw {raw} round {r}"
            job = _jobs(first, src)
            want = m.expand(src, moves, first)
            words = _words(env.expand(_dev(src), _dev(moves), first=first))
            assert np.array_equal(words, want), (what, [hex(w) for w in words], [hex(w) for w in want])
            assert not words[~job].any() and words[job].all()
            m.same_as(env, what)
            children = (first + np.nonzero(job)[0]).astype(np.int64)
            before = SM.everything(env)
            got = _words(env.rollout_jobs(_dev(children), 8, 2, SEED, RO.DIST_RANDOM, simple=0xF))
            want = m.rollout_jobs(children, 8, 2, SEED, RO.DIST_RANDOM, simple=0xF)
            assert np.array_equal(got, want), (what, "rollout_jobs", np.argwhere(got != want)[:4].tolist())
            assert SM.everything(env) == before, (what, "rollout_jobs changed the handle")
            if r in STEP_ROUNDS:
                m.step(STEP_MOVES[r])
                env.step_device(_dev(STEP_MOVES[r]))
                m.same_as(env, what + " step")
        if not raw:
            assert m.status["done"].any() and not m.status["done"].all()


@pytest.mark.gpu
def test_side_arrays_follow_the_copy_rule_with_end_of_tick_resets(hip_lib):
    """a POM_RESET_AT_END handle started as tests/test_expand.py::test_twin_handle_with_end_of_tick_resets starts its own (the envs in
    their second or third game, the episode counters and terminal records all different): three rounds with no step in between — a
    copying job's destination has its source's memory, episode counter and terminal record as they were before the call, and all three
    are unchanged everywhere else, the identity entries and the children that finish included"""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import RESET_AT_END
    start = pa.make_boards(N, seed=21)
    start["timeStep"] = np.array([0, 3, 14, 3])[np.arange(N) % 4]
    with _env(start, auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9) as env:
        env.step_simple(3, 46)
        seen_episodes = seen_terminal = finished = 0
        for r, (first, src, moves) in enumerate(ROUNDS[:3]):
            before = dict(memory=env.policy_memory(), episodes=env.episodes(), terminal=env.get_terminal_state())
            words = _words(env.expand(_dev(src), _dev(moves), first=first))
            job = _jobs(first, src)
            copied = job & (src != first + np.arange(len(src)))
            D, S = first + np.nonzero(copied)[0], src[copied]
            keep = np.ones(N, dtype=bool)
            keep[D] = False
            after = dict(memory=env.policy_memory(), episodes=env.episodes(), terminal=env.get_terminal_state())
            for k in after:
                assert after[k][D].tobytes() == before[k][S].tobytes(), (r, k, "a child's is not its source's")
                assert after[k][keep].tobytes() == before[k][keep].tobytes(), (r, k, "changed where nothing was copied")
            seen_episodes += int((before["episodes"][S] != before["episodes"][D]).sum())
            seen_terminal += sum(before["terminal"][s].tobytes() != before["terminal"][d].tobytes() for s, d in zip(S, D))
            finished += int(((words[job] & XO.RO_DONE) != 0).sum())
        assert seen_episodes > 0 and seen_terminal > 16 and finished > 0   # (the checks had something to see)


# ---- expand on a chaining handle, chained ticks before and after it ----------------------------------------------------------------

CN = 600


def _chain_list(first, count, seed, children=None):
    """sources spread over the whole batch with envs 0, 599 and 592 (the short last tile's first), repeats, identity entries, refused
    entries and a -1; `children`: slots of the expansion before, named by every third entry"""
    rng = np.random.default_rng(seed)
    outside = np.array([e for e in range(CN) if not first <= e < first + count])
    src = rng.choice(outside, count).astype(np.int64)
    if children is not None:
        src[::3] = rng.choice(children, len(src[::3]))
    src[[1, 17, 100]] = 0, 599, 592
    src[[4, 40, 77]] = src[2]                                   # a source four times
    for j in (7, 64, count - 1):
        src[j] = first + j                                      # identity
    src[10], src[90] = first + 11, first                        # refused: other slots of the range
    src[23] = -1
    return src, FC.random_moves(count, seed + 1)


C_FIRST1, C_FIRST2 = 203, 37
C_SRC1, C_MV1 = _chain_list(C_FIRST1, 151, 31)
C_SRC2, C_MV2 = _chain_list(C_FIRST2, 149, 33, children=C_FIRST1 + np.nonzero([XO.is_job(int(s), C_FIRST1 + j, C_FIRST1, 151, CN)
                                                                             for j, s in enumerate(C_SRC1)])[0])
C_CHILDREN = np.concatenate([C_FIRST1 + np.arange(3, 151, 6), C_FIRST2 + np.arange(0, 149, 5), [599, 0]]).astype(np.int64)
assert len(C_SRC1) % 16 and len(C_SRC2) % 16 and C_FIRST1 % 16 and C_FIRST2 % 16 and len(C_CHILDREN) % 16
assert sum(C_FIRST1 <= s < C_FIRST1 + 151 for s in C_SRC2) >= 40


@pytest.mark.gpu
@pytest.mark.parametrize("reset", ["at_start", "at_end"])
def test_expand_between_chained_launches(hip_lib, oracle, reset):
    """20 chained ticks, an expansion, 20 chained ticks, an expansion from children of the first, 9 chained ticks, rollout_jobs over
    children of both — on a handle that chains its launches, with no host read in between, and on one that issues them one by one:
    everything the API can read is the same at the end, and so are the three calls' words.  The expansion must wait for the chained
    launches before it (quiesce) and the chained launches after it must start from the children (they fork behind the handle's
    stream).  The plain handle, which may be read in between, is tied to the checker: its first expansion from a download before and
    after it, and (restarts at the start of a tick, the checker's rule) the ticks after either expansion"""
    import torch
    from pomcpp_amd.batch import ISSUE_CHAIN, ISSUE_THREADS, MODE_ENV, RESET_AT_END, RESET_AT_START
    auto_reset = RESET_AT_START if reset == "at_start" else RESET_AT_END
    states = FC.played_states(oracle, "stress", CN, 23)
    kw = dict(mode=MODE_ENV, auto_reset=auto_reset, max_steps=300)
    job1 = np.array([XO.is_job(int(s), C_FIRST1 + j, C_FIRST1, len(C_SRC1), CN) for j, s in enumerate(C_SRC1)])
    with _env(states, issue_mode=ISSUE_CHAIN, **kw) as a, _env(states, issue_mode=ISSUE_THREADS, streams=1, **kw) as b:
        assert a.issue_info()[0] == "chain" and b.issue_info()[0] != "chain"
        src1, mv1, src2, mv2, kids = _dev(C_SRC1), _dev(C_MV1), _dev(C_SRC2), _dev(C_MV2), _dev(C_CHILDREN)
        out = {}
        for env in (a, b):
            out[env] = (torch.full((len(C_SRC1),), -7, dtype=torch.int32, device="cuda"),
                        torch.full((len(C_SRC2),), -7, dtype=torch.int32, device="cuda"),
                        torch.full((2, len(C_CHILDREN)), -7, dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        for env in (a, b):
            env.step_random(5, RO.DIST_RANDOM, ticks=20)
            if env is b:
                before = env.get_state(), env.status()
            env.expand(src1, mv1, first=C_FIRST1, out=out[env][0])
            if env is b:
                after = env.get_state()
            env.step_random(5, RO.DIST_RANDOM, ticks=20)
            if env is b:
                mid = env.get_state()
            env.expand(src2, mv2, first=C_FIRST2, out=out[env][1])
            if env is b:
                after2 = env.get_state()
            env.step_random(6, RO.DIST_STRESS, ticks=9)
            env.rollout_jobs(kids, 8, 2, SEED, out=out[env][2], simple=0xF)
        last = b.get_state()
        ea, eb = SM.everything(a), SM.everything(b)
        stats = ea.pop("chain")
        eb.pop("chain")
        for k in ea:
            assert ea[k] == eb[k], (reset, k)
        for i, what in enumerate(("expansion 1", "expansion 2", "rollout_jobs")):
            wa, wb = _words(out[a][i]), _words(out[b][i])
            assert np.array_equal(wa, wb), (reset, what, np.argwhere(wa != wb)[:4].tolist())
            assert not (out[a][i] == -7).any()
        assert stats["launches"] == 49 and stats["tiles_recovered"] == 0, stats
        assert _words(out[a][2]).all() and (_words(out[a][0]) != 0).sum() == job1.sum()
    # the tie to the checker: the plain handle's first expansion, from what it held before.  (RESET_AT_END: no env stands finished
    # after a tick; RESET_AT_START: a finished env stands finished until its next tick, with the time-out the status does not report)
    st = SM.status_of(before[1], 300)
    want, _, want_words, _, _ = XO.expand(oracle, before[0], st, C_SRC1, C_MV1, C_FIRST1, XO.MODE_ENV, 300)
    D = C_FIRST1 + np.nonzero(job1)[0]
    assert after[D].tobytes() == want[D].tobytes(), reset
    assert np.array_equal(_words(out[b][0]), want_words), reset
    assert after.tobytes() == want.tobytes(), (reset, "an env without a job changed")
    if reset == "at_start":
        # ... and the plain handle's ticks after each expansion are the checker's, from the children: a finished child is restarted from
        # its slot's own snapshot on the next tick (the handle's tick, which keys the draws, is not moved by an expansion)
        for begin, end, ticks, seed, tick0, dist in ((after, mid, 20, 5, 20, RO.DIST_RANDOM), (after2, last, 9, 6, 40, RO.DIST_STRESS)):
            want = begin.copy()
            oracle.run_random(want, states, ticks, seed, 0, tick0, dist, 300)
            want["agents"]["pad"] = 0
            assert end.tobytes() == want.tobytes(), (tick0, "the ticks after an expansion did not start from the children")
