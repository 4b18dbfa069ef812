"""Where the list-driven kernels (pom_batch_expand, pom_batch_rollout_jobs: include/pom_batch.h) take a game from and put it: every
(source column, destination column) pair of the 16-env tiles in one launch each, every alignment of expand's destination range against
the tiles, lists that nearly are "16 envs of one tile in order" (the lists the kernels load as a tile instead of gathering), and the
envs the fused observation of an expansion writes — the touched tiles below n and nothing else.  All against the checkers
(tests/expand_oracle.py, tests/rollout_jobs_oracle.py), which know no tile and no column."""
import ctypes as C

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests import expand_oracle as XO
from tests import forecast_cases as FC
from tests import rollout_jobs_oracle as JO
from tests import rollout_oracle as RO
from tests.rollout_gpu import _dev, _env, _played, _same, _words

SEED = 99

# ---- all 256 (source column, destination column) pairs -------------------------------------------------------------------------------
# job j = 16 t + c (destination tile t, column c) takes env 16 ((3 c + t) % 16) + (c + t) % 16
PAIR_SRC = np.array([16 * ((3 * (j & 15) + (j >> 4)) % 16) + ((j & 15) + (j >> 4)) % 16 for j in range(256)], dtype=np.int64)
assert len({(int(s) & 15, j & 15) for j, s in enumerate(PAIR_SRC)}) == 256
assert len({(int(s) >> 4, j >> 4) for j, s in enumerate(PAIR_SRC)}) == 256               # ... and every (source tile, destination tile)
for _t in range(16):                                                                    # no tile's sources are one tile in order
    _s = PAIR_SRC[16 * _t:16 * _t + 16]
    assert not ((_s >> 4 == _s[0] >> 4).all() and (_s & 15 == np.arange(16)).all())


@pytest.fixture(scope="module")
def pair_states(oracle):
    s = FC.played_states(oracle, "ffa", 256, 57)
    assert len({s[e].tobytes() for e in range(256)}) == 256
    s.setflags(write=False)
    return s


@pytest.mark.gpu
def test_expand_every_column_pair(hip_lib, oracle, pair_states):
    """256 distinct games in envs 0..255 of a RAW handle, their children in envs 256..511 through the list above: the children are the
    checker's, the sources byte for byte as before"""
    from pomcpp_amd.batch import MODE_RAW
    states = np.concatenate([pair_states, np.zeros(256, dtype=STATE_DTYPE)])
    moves = FC.random_moves(256, 17)
    want, _, want_words, ticks, _ = XO.expand(oracle, states, None, PAIR_SRC, moves, 256, XO.MODE_RAW)
    with _env(states, mode=MODE_RAW) as env:
        words = _words(env.expand(PAIR_SRC, moves, first=256))
        got = env.get_state()
        assert env.counters().tolist()[:3] == [256, 0, 0] and ticks == 256
    bad = [j for j in range(256) if got[256 + j].tobytes() != want[256 + j].tobytes()]
    assert not bad, f"children differ from the checker's, (source column, destination column) {[(int(PAIR_SRC[j]) & 15, j & 15) for j in bad[:8]]}"
    assert np.array_equal(words, want_words)
    assert got[:256].tobytes() == pair_states.tobytes(), "a source changed"


@pytest.mark.gpu
def test_rollout_jobs_every_column_pair(hip_lib, oracle, pair_states):
    """the same list on the 256-env batch: 16 groups of jobs, every source column in every column of a group"""
    moves = FC.random_moves(256, 19)
    want = JO.rollout_jobs(oracle, pair_states, None, PAIR_SRC, 8, 1, SEED, RO.DIST_RANDOM, 0x5, 0x2, moves)
    with _env(pair_states) as env:
        got = env.rollout_jobs(_dev(PAIR_SRC), 8, 1, SEED, RO.DIST_RANDOM, moves=_dev(moves), simple=0x5, first=0x2)
        _same(got, want, "every column pair")
        assert env.get_state().tobytes() == pair_states.tobytes()
    assert want.all() and len(set(want[0].tolist())) > 16


# ---- every alignment of the destination range ------------------------------------------------------------------------------------------
N = 72
ALIGN_FIRSTS, ALIGN_COUNTS = range(16, 32), (1, 15, 16, 17, 33)


def _align_list(first, count, rng):
    """sources outside the range — one of them out of a destination tile where the range leaves one — an identity entry and a -1"""
    inside = range(first, first + count)
    outside = np.array([e for e in range(N) if e not in inside])
    tiles = range(first // 16, (first + count - 1) // 16 + 1)
    near = np.array([e for t in tiles for e in range(16 * t, min(16 * t + 16, N)) if e not in inside])
    src = rng.choice(outside, count).astype(np.int64)
    pos = rng.permutation(count)
    if near.size:
        src[pos[0]] = rng.choice(near)
    if count > 1:
        src[pos[1]] = first + pos[1]
    if count > 2:
        src[pos[2]] = -1
    return src


@pytest.mark.gpu
def test_expand_at_every_range_alignment(hip_lib, oracle):
    """first = 16..31 x count = 1, 15, 16, 17, 33: a range that begins and ends at every column, inside one tile, over a boundary, over
    a whole tile and more.  80 calls on one handle, the checker carried from call to call: after each the whole batch, the statuses and
    the words are the checker's"""
    rng = np.random.default_rng(13)
    states, status = _played("stress", 23)[:N].copy(), None
    seen_near = 0
    with _env(states) as env:
        counters = [0, 0, 0]
        for first in ALIGN_FIRSTS:
            for count in ALIGN_COUNTS:
                src, moves = _align_list(first, count, rng), FC.random_moves(count, 1000 + 40 * first + count)
                seen_near += any((first >> 4) * 16 <= s < first or first + count <= s < ((first + count - 1) >> 4) * 16 + 16 for s in src)
                states, status, want_words, ticks, newly = XO.expand(oracle, states, status, src, moves, first, XO.MODE_ENV)
                counters[0] += ticks
                counters[1] += newly
                words = _words(env.expand(src, moves, first=first))
                what = f"first {first} count {count}"
                assert np.array_equal(words, want_words), (what, [hex(w) for w in words], [hex(w) for w in want_words])
                got, st = env.get_state(), env.status()
                bad = [e for e in range(N) if got[e].tobytes() != states[e].tobytes()]
                assert not bad, (what, "envs that differ from the checker's", bad)
                for k in ("done", "winner", "draw", "ubflags"):
                    assert np.array_equal(st[k], status[k]), (what, k)
                assert env.counters().tolist()[:3] == counters, what
    assert seen_near >= 70 and not status["done"].all()


# ---- lists that nearly are one tile in order ----------------------------------------------------------------------------------------------

def _near_misses():
    base = np.arange(32, 48, dtype=np.int64)
    swapped, none, repeat = base.copy(), base.copy(), base.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    none[0] = -1
    repeat[15] = 32
    return {"in order": base, "3 and 4 swapped": swapped, "entry 0 is -1": none, "entry 15 repeats 32": repeat,
            "two tiles": np.arange(40, 56, dtype=np.int64), "reversed": base[::-1].copy()}


NEAR = _near_misses()


@pytest.mark.gpu
def test_expand_lists_that_nearly_are_a_tile(hip_lib, oracle):
    """destination tile 1 (envs 16..31) filled from tile 2, in order — the list the kernel loads as a tile — and the lists one entry
    away from it, which it must gather; then the in-order list over 15 of the tile's 16 columns, at either end.  One handle, the
    checker carried along; a destination without a job keeps its bytes"""
    states, status = _played("stress", 23)[:N].copy(), None
    cases = [(what, 16, src) for what, src in NEAR.items()]
    cases += [("columns 0..14", 16, np.arange(32, 47, dtype=np.int64)), ("columns 1..15", 17, np.arange(33, 48, dtype=np.int64))]
    with _env(states) as env:
        for k, (what, first, src) in enumerate(cases):
            moves = FC.random_moves(len(src), 50 + k)
            before = states
            states, status, want_words, _, _ = XO.expand(oracle, states, status, src, moves, first, XO.MODE_ENV)
            words = _words(env.expand(src, moves, first=first))
            got, st = env.get_state(), env.status()
            bad = [e for e in range(N) if got[e].tobytes() != states[e].tobytes()]
            assert not bad, (what, "envs that differ from the checker's", bad)
            assert np.array_equal(words, want_words), what
            for key in ("done", "winner", "draw", "ubflags"):
                assert np.array_equal(st[key], status[key]), (what, key)
            idle = [e for e in range(16, 32) if not (first <= e < first + len(src) and src[e - first] >= 0)]
            assert all(got[e].tobytes() == before[e].tobytes() for e in idle), what
            assert len(idle) == {"entry 0 is -1": 1, "columns 0..14": 1, "columns 1..15": 1}.get(what, 0)


@pytest.mark.gpu
def test_rollout_jobs_lists_that_nearly_are_a_tile(hip_lib, oracle):
    """the same groups of 16 as lists of jobs, and the in-order list cut to 15 (the group's last slot lies past the list's end)"""
    states = _played("stress", 23)[:N].copy()
    cases = dict(NEAR)
    cases["a list of 15"] = np.arange(32, 47, dtype=np.int64)
    with _env(states) as env:
        for k, (what, src) in enumerate(cases.items()):
            moves = FC.random_moves(len(src), 70 + k)
            want = JO.rollout_jobs(oracle, states, None, src, 8, 1, SEED, RO.DIST_STRESS, 0x5, 0x2, moves)
            got = env.rollout_jobs(_dev(src), 8, 1, SEED, RO.DIST_STRESS, moves=_dev(moves), simple=0x5, first=0x2)
            _same(got, want, what)
            assert np.array_equal(want[0] != 0, src >= 0), what
        assert env.get_state().tobytes() == states.tobytes()


# ---- the fused observation: the touched tiles below n, nothing else --------------------------------------------------------------------------
GUARD = 0xA5
FORMS = {"codes": (3, 0, 5 * 121), "planes": (0, 0, 16 * 121), "per_agent_f16": (1, 1, 4 * 16 * 121 * 2)}   # dtype, per_agent, bytes per env


@pytest.mark.gpu
@pytest.mark.parametrize("first,count", [(19, 18), (60, 12)])
@pytest.mark.parametrize("form", list(FORMS))
def test_observation_writes_the_touched_tiles_only(hip_lib, oracle, form, first, count):
    """through the C ABI, so that the three outputs can lie inside larger guard-filled buffers with room for 16 more envs behind env
    n - 1: the touched tiles' envs below n hold what observe() writes afterwards; every byte of the tiles below and above the range is
    the guard's, and so is every byte behind env n - 1 — the range 60..71 ends in the short tile, whose columns 72..79 lie past the
    batch's end but are in the wavefront's LDS tile like any other"""
    import torch
    from pomcpp_amd.batch import _check, _ExpandSpec as Spec
    code, per_agent, env_bytes = FORMS[form]
    lead, tail = 256, 16
    rng = np.random.default_rng(first)
    outside = np.array([e for e in range(N) if not first <= e < first + count])
    src, moves = rng.choice(outside, count).astype(np.int64), FC.random_moves(count, first)
    src[2] = -1
    states = _played("ffa", 57)[:N].copy()
    with _env(states) as env:
        assert env.device_view()[1] == 128
        bufs = {k: torch.full((lead + (N + tail) * b + lead,), GUARD, dtype=torch.uint8, device="cuda")
                for k, b in (("planes", env_bytes), ("agent", 4 * 8 * 4), ("env", 4 * 4))}
        ptr = {k: v.data_ptr() + lead for k, v in bufs.items()}
        assert all(p % 16 == 0 for p in ptr.values())
        s, m = _dev(src), _dev(moves)
        words = torch.zeros(count, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        spec = Spec(C.sizeof(Spec), 0, first, count, s.data_ptr(), m.data_ptr(), words.data_ptr(), ptr["planes"], code, per_agent,
                    ptr["agent"], ptr["env"], 0)
        _check(env._lib, env._lib.pom_batch_expand(env._h, C.byref(spec)))
        env.sync()
        want = env.observe(per_agent=bool(per_agent), dtype={3: "codes", 0: "uint8", 1: "float16"}[code])
        touched = range(16 * (first // 16), min(N, 16 * ((first + count - 1) // 16) + 16))
        # (the batch and the words are the checker's with the observation fused in as without: the range 60..71 ends at the batch's end)
        checked, _, want_words, _, _ = XO.expand(oracle, states, None, src, moves, first, XO.MODE_ENV)
        assert env.get_state().tobytes() == checked.tobytes() and np.array_equal(_words(words), want_words)
        assert (want_words != 0).sum() == count - 1
        for (k, buf), w in zip(bufs.items(), want):
            b = w.numel() * w.element_size() // N
            got = buf.cpu().numpy()
            ref = w.contiguous().view(torch.uint8).reshape(N, b).cpu().numpy()
            body = got[lead:lead + N * b].reshape(N, b)
            for e in range(N):
                if e in touched:
                    assert np.array_equal(body[e], ref[e]), (form, k, "env", e, "is not observe()'s")
                else:
                    assert (body[e] == GUARD).all(), (form, k, "env", e, "of an untouched tile was written")
            assert (got[:lead] == GUARD).all(), (form, k, "bytes before env 0 were written")
            behind = got[lead + N * b:]
            assert behind.size >= 16 * b and (behind == GUARD).all(), (form, k, "bytes behind env n - 1 were written",
                                                                       np.nonzero(behind != GUARD)[0][:8].tolist())
