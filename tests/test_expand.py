"""pom_batch_expand on the GPU (include/pom_batch.h PomExpandSpec): env first + j becomes the successor of env src[j] under moves[j],
bit-exact against the compiled reference's recorded steps (tests/golden/step_cases.npz), the checker (tests/expand_oracle.py) and a twin
handle that does it the old way (copy_envs, then step_device); the masked step, the fused observation, and the intended use — expand,
then rollout_jobs over the new slots.

The batch is 40 envs — two whole tiles and a short one of 8, n_pad 64 — and the destination range first = 19, count = 18: two tiles, both
partly (columns 3..15 of tile 1, 0..4 of tile 2).  The list holds sources from all three tiles, sources in both destination tiles but
outside the range (16, 17, 18, 37, 38, 39), source 5 three times with different move rows, two identity entries (25, 33), one refused
in-range foreign source (20), and -1, n, n_pad - 1 and 2^40: 13 jobs and 5 entries without one."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import expand_oracle as XO
from tests import forecast_cases as FC
from tests.rollout_gpu import _dev, _env, _played, _words

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "step_cases.npz")

N, N_PAD, FIRST, COUNT = 40, 64, 19, 18
SRC = np.array([0, 17, 38, 5, 5, -1, 25, 20, 40, 63, 1 << 40, 16, 39, 5, 33, 2, 37, 18], dtype=np.int64)
DEST = FIRST + np.arange(COUNT)
JOB = np.array([XO.is_job(int(s), int(d), FIRST, COUNT, N) for s, d in zip(SRC, DEST)])
MOVES = FC.random_moves(COUNT, 41)
SRC_VALID = np.where(JOB, SRC, -1)                       # what copy_envs is given on the twin handle
KINDS = [("ffa", 57), ("stress", 23)]

assert SRC.size == COUNT and N_PAD - 1 == 63 and JOB.sum() == 13 and (~JOB).sum() == 5
assert len({tuple(MOVES[j]) for j in np.nonzero(SRC == 5)[0]}) == 3


def _full_moves(rows=MOVES, first=FIRST, n=N):
    """step_device's array for the twin handle: the jobs' rows at their destinations"""
    mv = np.zeros((n, 4), dtype=np.int32)
    mv[first:first + len(rows)] = rows
    return mv


def _status_equal(got, want, states, where=slice(None), what=""):
    for k in ("done", "winner", "draw"):
        assert np.array_equal(got[k][where], want[k][where]), (what, k)
    assert np.array_equal(got["ubflags"][where], want["ubflags"][where]), (what, "ubflags")
    assert np.array_equal(got["alive"][where], states["aliveAgents"][where]) and np.array_equal(got["time_step"][where], states["timeStep"][where]), what


@pytest.mark.gpu
def test_reference_fixture(hip_lib):
    """every Step the compiled reference recorded, as an expansion on a RAW handle: the `__before` states in the lower part (several
    tiles), their children in the upper part through a permuted list — with one destination tile whose 16 sources are one tile in order,
    the path that loads the source tile as a tile — compared the way tests/test_step_function.py compares GPU states; the sources
    are unchanged"""
    from pomcpp_amd.batch import MODE_RAW
    g = np.load(GOLDEN)
    names = sorted(k[:-len("__before")] for k in g.files if k.endswith("__before"))
    before = np.concatenate([g[f"{k}__before"] for k in names]).view(STATE_DTYPE).reshape(-1)
    after = np.concatenate([g[f"{k}__after"] for k in names]).view(STATE_DTYPE).reshape(-1)
    moves = np.concatenate([g[f"{k}__moves"] for k in names]).astype(np.int32)
    m = before.size
    assert m == 219 and m % 16 != 0
    # destination tile 14 = envs 224..239 = entries 5..20 of the list: their sources are envs 32..47, in order
    rest = np.random.default_rng(5).permutation(np.concatenate([np.arange(32), np.arange(48, m)]))
    perm = np.concatenate([rest[:5], np.arange(32, 48), rest[5:]]).astype(np.int64)
    assert sorted(perm.tolist()) == list(range(m)) and (m + 5) % 16 == 0
    with _env(np.concatenate([before, np.zeros(m, dtype=STATE_DTYPE)]), mode=MODE_RAW) as env:
        words = _words(env.expand(perm, moves[perm], first=m))
        got = env.get_state()
        assert env.counters().tolist()[:3] == [m, 0, 0]
    assert got[m:].tobytes() == after[perm].tobytes(), "children differ from the reference's states after the step"
    assert got[:m].tobytes() == before.tobytes(), "a source changed"
    assert ((words >> XO.RO_LENGTH_SHIFT) == 1).all() and not (words & (XO.RO_DONE | XO.RO_DRAW | XO.RO_TIMEOUT | 0x700)).any()
    alive = np.stack([1 - after["agents"]["dead"][perm][:, a].astype(np.int64) for a in range(4)], axis=1) @ (1 << np.arange(4))
    assert np.array_equal(words & 0xF, alive)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bound", [False, True])
@pytest.mark.parametrize("raw", [True, False])
@pytest.mark.parametrize("kind,ticks", KINDS)
def test_matches_the_checker(hip_lib, oracle, kind, ticks, raw, with_bound):
    """the hand-built list on mid-game boards: the whole downloaded batch, the statuses and the words are the checker's; the entries
    without a job give 0 and leave their env as it was.  With max_steps = ticks + 1 (the boards' timeStep set to `ticks`: the pool's
    games have restarted at various ticks) every ticked child comes back DONE | TIMEOUT in ENV mode.  A second expansion from where the
    first left off then meets finished sources (the identity entries): unticked, length 0."""
    from pomcpp_amd.batch import MODE_ENV, MODE_RAW
    mode, max_steps = (MODE_RAW if raw else MODE_ENV), (ticks + 1 if with_bound else 0)
    states = _played(kind, ticks)[:N].copy()
    if with_bound:
        states["timeStep"] = ticks
    status = None
    with _env(states, mode=mode, max_steps=max_steps) as env:
        assert env.device_view()[1] == N_PAD
        src, mv = _dev(SRC), _dev(MOVES)
        for rnd in range(2):
            want, status, want_words, ticked, newly = XO.expand(oracle, states, status, SRC, MOVES, FIRST, mode, max_steps)
            c0 = env.counters()
            words = _words(env.expand(src, mv, first=FIRST))
            got, c1 = env.get_state(), env.counters()
            what = f"{kind} raw {raw} max_steps {max_steps} round {rnd}"
            assert np.array_equal(words, want_words), (what, [hex(w) for w in words], [hex(w) for w in want_words])
            assert got.tobytes() == want.tobytes(), what
            _status_equal(env.status(), status, want, what=what)
            assert not words[~JOB].any() and words[JOB].all()
            keep = np.ones(N, dtype=bool)
            keep[DEST[JOB]] = False                          # envs outside the range and the destinations without a job
            assert got[keep].tobytes() == states[keep].tobytes(), what
            assert (c1 - c0).tolist()[:3] == [ticked, newly, 0], what
            length = words[JOB] >> XO.RO_LENGTH_SHIFT
            if raw or rnd == 0:
                assert ticked == 13 and (length == 1).all()
            if with_bound and not raw:
                t = (words >> XO.RO_LENGTH_SHIFT) == 1
                assert ((words[t] & (XO.RO_DONE | XO.RO_TIMEOUT)) == (XO.RO_DONE | XO.RO_TIMEOUT)).all()
                if rnd == 1:                                 # the identity entries' games finished in round 0
                    assert (length[np.isin(SRC[JOB], (25, 33))] == 0).all() and ticked == 11
            states = want
        assert np.array_equal(src.cpu().numpy(), SRC) and np.array_equal(mv.cpu().numpy(), MOVES)


def _twin_step(states, prepare, **kw):
    """handle A expands, handle B copies the valid sources and steps the whole batch with the jobs' rows; both after `prepare`"""
    a, b = _env(states, **kw), _env(states, **kw)
    for env in (a, b):
        prepare(env)
    before = dict(state=a.get_state(), status=a.status(), memory=a.policy_memory(), episodes=a.episodes())
    words = _words(a.expand(_dev(SRC), _dev(MOVES), first=FIRST))
    b.copy_envs(SRC_VALID, first=FIRST)
    b.step_device(_dev(_full_moves()))
    return a, b, before, words


@pytest.mark.gpu
def test_twin_handle_with_agent_memory(hip_lib):
    """in the middle of SimpleAgent games (the agents' memory is not zero): A's job destinations are B's — state, status, agent memory,
    episode counter — and everything else of A is as before"""
    import pomcpp_amd as pa
    a, b, before, words = _twin_step(pa.make_boards(N, seed=21), lambda env: env.step_simple(3, 40))
    with a, b:
        D = DEST[JOB]
        assert before["memory"][SRC[JOB]].any()
        sa, sb = a.get_state(), b.get_state()
        assert sa[D].tobytes() == sb[D].tobytes()
        ga, gb = a.status(), b.status()
        for k in ga:
            assert np.array_equal(ga[k][D], gb[k][D]), k
        assert a.policy_memory()[D].tobytes() == b.policy_memory()[D].tobytes() == before["memory"][SRC[JOB]].tobytes()
        assert np.array_equal(a.episodes()[D], b.episodes()[D])
        keep = np.ones(N, dtype=bool)
        keep[D] = False
        assert sa[keep].tobytes() == before["state"][keep].tobytes() and a.policy_memory()[keep].tobytes() == before["memory"][keep].tobytes()
        assert np.array_equal(words[JOB] >> XO.RO_LENGTH_SHIFT, 1 - before["status"]["done"][SRC[JOB]])


@pytest.mark.gpu
def test_twin_handle_with_end_of_tick_resets(hip_lib):
    """a POM_RESET_AT_END handle with fresh boards, 46 ticks into SimpleAgent games bounded at 25 ticks whose first games started at
    timeStep 0, 3, 14, 3 (env % 4): the envs stand at 21, 24, 10, 24 in their second or third game — the children of the odd ones time
    out, and sources and destinations differ in their episode counters.  Children that do not finish are B's in every array, last results
    and terminal record included; a child that finishes STAYS finished, is not marked restarted, keeps its source's episode counter and
    terminal record, and its state is the final state B filed as the terminal record"""
    import pomcpp_amd as pa
    from pomcpp_amd.batch import RESET_AT_END
    start = pa.make_boards(N, seed=21)
    start["timeStep"] = np.array([0, 3, 14, 3])[np.arange(N) % 4]
    kw = dict(auto_reset=RESET_AT_END, max_steps=25, fresh_boards=True, board_seed=9)
    a, b, before, words = _twin_step(start, lambda env: env.step_simple(3, 46), **kw)
    with a, b:
        D, S = DEST[JOB], SRC[JOB]
        assert not before["status"]["done"].any() and (before["episodes"][S] != before["episodes"][D]).any()
        done = (words[JOB] & XO.RO_DONE) != 0
        assert done.any() and (~done).any() and ((words[JOB] >> XO.RO_LENGTH_SHIFT) == 1).all()
        assert done[before["state"]["timeStep"][S] == 24].all()
        sa, sb, ga, gb = a.get_state(), b.get_state(), a.status(), b.status()
        la, lb, ta, tb = a.last_results(), b.last_results(), a.get_terminal_state(), b.get_terminal_state()
        live = D[~done]
        assert sa[live].tobytes() == sb[live].tobytes() and ta[live].tobytes() == tb[live].tobytes()
        for k in ga:
            assert np.array_equal(ga[k][live], gb[k][live]), k
        for k in la:
            assert np.array_equal(la[k][live], lb[k][live]), k
        assert a.policy_memory()[D].tobytes() == before["memory"][S].tobytes() and a.policy_memory()[live].tobytes() == b.policy_memory()[live].tobytes()
        assert np.array_equal(a.episodes()[D], before["episodes"][S]) and np.array_equal(a.episodes()[live], b.episodes()[live])
        fin = D[done]
        assert (ga["done"][fin] == 1).all() and (la["finished"][fin] == 0).all() and (lb["finished"][fin] == 1).all()
        assert sa[fin].tobytes() == tb[fin].tobytes(), "a finished child is the final state the twin filed"
        assert np.array_equal(b.episodes()[fin], before["episodes"][S[done]] + 1)
        # ... and its terminal record is its source's, as copy_envs leaves it
        with _env(start, **kw) as c:
            c.step_simple(3, 46)
            t_before = c.get_terminal_state()
        assert t_before.tobytes() != np.zeros(N, dtype=STATE_DTYPE).tobytes() and ta[D].tobytes() == t_before[S].tobytes()
        # later ordinary steps skip a finished child (POM_RESET_AT_END restarts at the end of the tick that finishes, never later)
        a.step_device(_dev(_full_moves()))
        assert a.get_state()[fin].tobytes() == sa[fin].tobytes() and (a.status()["done"][fin] == 1).all()


@pytest.mark.gpu
def test_masked_step(hip_lib):
    """first = 0, count = n, an identity list with a few -1: the listed envs are step_device's on a twin, the others untouched; and the
    counters grow by exactly the ticks played and the children newly done, no reset"""
    states = _played("stress", 23)[:N].copy()
    src = np.arange(N, dtype=np.int64)
    off = np.array([0, 7, 16, 17, 30, 39])
    src[off] = -1
    moves = FC.random_moves(N, 9)
    with _env(states, max_steps=12) as a, _env(states, max_steps=12) as b:
        a.step_random(5, 1, ticks=1)                           # (some games are finished when the masked step begins)
        b.step_random(5, 1, ticks=1)
        mid, mid_status = a.get_state(), a.status()
        assert 0 < mid_status["done"].sum() < N
        c0 = a.counters()
        words = _words(a.expand(src, moves))
        c1 = a.counters()
        b.step_device(_dev(moves))
        sa, sb, ga, gb = a.get_state(), b.get_state(), a.status(), b.status()
        on = src >= 0
        assert sa[on].tobytes() == sb[on].tobytes() and sa[~on].tobytes() == mid[~on].tobytes()
        for k in ga:
            assert np.array_equal(ga[k][on], gb[k][on]) and np.array_equal(ga[k][~on], mid_status[k][~on]), k
        assert not words[~on].any() and words[on].all()
        ticked = (words >> XO.RO_LENGTH_SHIFT) == 1
        newly = ticked & ((words & XO.RO_DONE) != 0)
        assert np.array_equal(ticked[on], mid_status["done"][on] == 0) and newly.any()
        assert (c1 - c0).tolist() == [int(ticked.sum()), int(newly.sum()), 0, int(((words & XO.RO_UB) != 0).sum())]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["codes", "planes", "per_agent_f16"])
def test_observation(hip_lib, form):
    """the bytes of envs 16..39 — the two destination tiles — are what observe() writes afterwards, attributes included; the bytes of
    envs 0..15 of a pre-filled tensor are untouched; the guard words around the result are untouched"""
    import torch
    with _env(_played("ffa", 57)[:N].copy()) as env:
        shape, tdt, kw = {"codes": ((N, 5, 11, 11), torch.uint8, dict(dtype="codes")),
                          "planes": ((N, 16, 11, 11), torch.uint8, dict(dtype="uint8")),
                          "per_agent_f16": ((N, 4, 16, 11, 11), torch.float16, dict(dtype="float16", per_agent=True))}[form]
        out = torch.full(shape, 0xAB if tdt == torch.uint8 else 77.0, dtype=tdt, device="cuda")
        buf = torch.full((4 + COUNT + 4,), -7, dtype=torch.int32, device="cuda")
        res = env.expand(_dev(SRC), _dev(MOVES), first=FIRST, out=buf[4:4 + COUNT], per_agent=form == "per_agent_f16",
                         **({"codes": out} if form == "codes" else {"planes": out}))
        words, a_attrs, e_attrs = res
        assert words.data_ptr() == buf[4:].data_ptr() and (buf[:4] == -7).all() and (buf[4 + COUNT:] == -7).all() and not (words == -7).any()
        want, wa, we = env.observe(**kw)
        assert torch.equal(out[16:], want[16:]) and torch.equal(a_attrs[16:], wa[16:]) and torch.equal(e_attrs[16:], we[16:])
        assert (out[:16] == (0xAB if tdt == torch.uint8 else 77.0)).all()
        # ... and without attributes, the same planes
        out2 = torch.zeros_like(out)
        w2, a2, e2 = env.expand(_dev(SRC_VALID), _dev(MOVES), first=FIRST, attrs=False, per_agent=form == "per_agent_f16",
                                **({"codes": out2} if form == "codes" else {"planes": out2}))
        assert a2 is None and e2 is None and torch.equal(out2[16:], env.observe(**kw)[0][16:]) and not out2[:16].any()


@pytest.mark.gpu
def test_expand_then_evaluate(hip_lib):
    """the intended use: the children of a list of parents in one launch, valued in the next — rollout_jobs over the new slots gives
    the words it gives on the twin handle's copies"""
    states = _played("ffa", 57)[:N].copy()
    with _env(states) as a, _env(states) as b:
        a.expand(SRC, MOVES, first=FIRST)
        b.copy_envs(SRC_VALID, first=FIRST)
        b.step_device(_dev(_full_moves()))
        slots = _dev(DEST[JOB].astype(np.int64))
        got = _words(a.rollout_jobs(slots, 24, 2, 99, simple=0xF))
        assert np.array_equal(got, _words(b.rollout_jobs(slots, 24, 2, 99, simple=0xF))) and got.all()


@pytest.mark.gpu
def test_bad_arguments_are_refused(hip_lib):
    """what needs a live handle: ranges outside the batch, the observation's own checks, a handle of another launch shape; an empty list
    is OK and writes nothing; the wrapper's own checks"""
    import torch
    from pomcpp_amd.batch import PomError, _check, _ExpandSpec as Spec
    with _env(_played("ffa", 57)[:N].copy()) as env, _env(_played("ffa", 57)[:N].copy(), envs_per_wave=32, lanes_per_env=1) as one:
        lib = env._lib
        s, m = _dev(SRC), _dev(MOVES)
        r = torch.full((COUNT,), -7, dtype=torch.int32, device="cuda")
        codes = torch.zeros((N, 5, 11, 11), dtype=torch.uint8, device="cuda")
        size = C.sizeof(Spec)
        before = env.get_state().tobytes()

        def spec(first=FIRST, count=COUNT, planes=None, dtype=0, per_agent=0, a=None, e=None):
            return Spec(size, 0, first, count, s.data_ptr(), m.data_ptr(), r.data_ptr(), planes, dtype, per_agent, a, e, 0)

        bad = {"first < 0": (env, spec(first=-1)), "past the end": (env, spec(first=N - COUNT + 1)), "first > n": (env, spec(first=N + 1, count=0)),
               "count beyond int64": (env, spec(first=1, count=(1 << 63) - 1)),
               "codes per agent": (env, spec(planes=codes.data_ptr(), dtype=3, per_agent=1)),
               "planes + 4": (env, spec(planes=codes.data_ptr() + 4, dtype=0)),
               "attrs + 4": (env, spec(planes=codes.data_ptr(), dtype=3, a=codes.data_ptr() + 4)),
               "one lane per env": (one, spec())}
        for what, (handle, sp) in bad.items():
            with pytest.raises(PomError) as err:
                _check(lib, lib.pom_batch_expand(handle._h, C.byref(sp)))
            assert err.value.code == 1 and "pom_batch_expand" in str(err.value), what
        _check(lib, lib.pom_batch_expand(env._h, C.byref(spec(count=0))))
        _check(lib, lib.pom_batch_expand(env._h, C.byref(spec(first=N, count=0))))
        empty = env.expand(s[:0], m[:0], first=7)
        assert tuple(empty.shape) == (0,)
        env.sync()
        assert (r == -7).all() and not codes.any() and env.get_state().tobytes() == before
        for args, kw in (((s.to(torch.int32), m), {}), ((s, m.to(torch.int64)), {}), ((s, m[:COUNT - 1]), {}), ((s.cpu(), m), {}),
                         ((s, m), dict(first=N - COUNT + 1)), ((s, m), dict(out=r[:COUNT - 1])), ((s, m), dict(codes=codes, planes=codes)),
                         ((s, m), dict(codes=codes, per_agent=True)), ((s, m), dict(planes=codes))):
            with pytest.raises(ValueError):
                env.expand(*args, first=kw.pop("first", FIRST), **kw)
