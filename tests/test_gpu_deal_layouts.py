"""pom_batch_deal on the GPU beyond the standard layout (include/pom_batch.h PomDealSpec).  The curricula, POM_LAYOUT_NO_LANES,
POM_DEAL_FALLBACK, game numbers at the ends of int32 and an env_offset that crosses the uint32 wrap of the key have only run on the
host build of the rule functions, which has its own quad type; the device's PomQuadLanes gathers by DPP and floods inside `if (todo)`,
where the quads of one wavefront need different numbers of attempts.  Here ten layouts are dealt into 77 envs (four tiles and a short
one of 13) at three env_offsets and compared byte for byte with the checker (tests/deal_oracle.py): States, result words, game counters,
the restart snapshots seen through restore(), and what a call must leave alone."""
import numpy as np
import pytest

from tests import deal_oracle as DO
from tests.test_deal_host import CURRICULA, check_invariants

N, SEED = 77, 20261020
MIXED = (56, 24, 10, 2, DO.NO_LANES)   # every tile of 16 holds fallback boards beside boards accepted after different numbers of attempts
LAYOUTS = [DO.STANDARD] + [c[0] for c in CURRICULA] + [(80, 0, 0, 121, DO.NO_LANES), (0, 80, 80, 4, DO.NO_LANES), (0, 0, 0, 0, DO.NO_LANES),
                                                       (56, 36, 36, 4, 0), (56, 24, 10, 0, DO.NO_LANES), MIXED]
OFFSETS = [0, 10 ** 6, 2 ** 32 - 40]   # the last: env_offset + e passes 2^32 inside the batch
GAMES = [0, 1, 7, 2 ** 31 - 1, -2 ** 31, -1]
SENTINEL = 0x5A5A5A5A
gpu = pytest.mark.gpu


def start_games():
    return np.resize(np.array(GAMES, dtype=np.int64), N).astype(np.int32)


def next_mask():
    """the envs deal(NEXT, MASK) takes: another subset of columns in every tile — tile 1 none, tile 2 its last column only, the short
    tile its first and its last (column 12) among others"""
    mask = np.zeros(N, dtype=bool)
    mask[[0, 3, 4, 9, 14]] = True
    mask[32 + 15] = True
    mask[48 + np.array([1, 2, 5, 6, 7, 8, 10, 11, 12, 13, 15])] = True
    mask[64 + np.array([0, 5, 7, 12])] = True
    return mask


def per_tile(words):
    """[(fallbacks, accepted, distinct attempt counts)] of the tiles of 16 envs"""
    fallback, attempts = (words & DO.FALLBACK) != 0, (words >> DO.ATTEMPTS_SHIFT) & 0xFF
    return [(int(fallback[k:k + 16].sum()), int((~fallback[k:k + 16]).sum()), len(set(attempts[k:k + 16].tolist()))) for k in range(0, len(words), 16)]


# ---- no GPU: what the placements and the mixed layout give, recounted from the checker ------------------------------------------------
def test_the_mask_takes_another_subset_of_every_tile():
    mask, g = next_mask(), start_games()
    subsets = [tuple(np.flatnonzero(mask[k:k + 16]).tolist()) for k in range(0, N, 16)]
    assert len(set(subsets)) == 5 and subsets[1] == () and subsets[2] == (15,) and 12 in subsets[4] and N - 1 == 64 + 12
    assert all(0 < len(s) < 16 for s in (subsets[0], subsets[3], subsets[4]))
    assert set(g.tolist()) == set(GAMES) and DO.next_game(g)[g == 2 ** 31 - 1].tolist() == [-2 ** 31] * int((g == 2 ** 31 - 1).sum())
    assert (OFFSETS[2] + np.arange(N) >= 2 ** 32).any() and (OFFSETS[2] + np.arange(N) < 2 ** 32).any()


@pytest.fixture(scope="module")
def mixed_words():
    """the checker's words of the mixed layout, game 0, at env_offset 0 and 2^32 - 40"""
    return {offset: DO.deal_many(SEED, np.arange(N), np.zeros(N, dtype=np.int64), MIXED, offset)[1] for offset in (0, 2 ** 32 - 40)}


def test_the_mixed_layout_diverges_in_every_tile(mixed_words):
    """every tile holds 4 to 10 fallback boards beside accepted boards with at least 5 distinct attempt counts — measured; what is
    required: a fallback, an accepted board and 3 distinct attempt counts in every tile, so that the attempt loop diverges in every wavefront"""
    for offset, words in mixed_words.items():
        tiles = per_tile(words)
        print(offset, tiles)
        assert len(tiles) == 5 and all(f >= 1 and a >= 1 and d >= 3 for f, a, d in tiles), (offset, tiles)
    words = DO.deal_many(SEED, np.arange(N), np.zeros(N, dtype=np.int64), (56, 24, 10, 0, DO.NO_LANES))[1]
    assert ((words & DO.FALLBACK) != 0).sum() >= 70   # 16 attempts nearly everywhere


# ---- the GPU ----------------------------------------------------------------------------------------------------------------------
def _handle(offset):
    import pomcpp_amd as pa
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV
    start = pa.make_boards(N, seed=8)
    env = BatchEnvironment(N, mode=MODE_ENV, max_steps=25, env_offset=offset)
    env.make_game(start)
    return env, start


def _layout(layout):
    import pomcpp_amd as pa
    return pa.BoardLayout(*layout[:4], no_lanes=bool(layout[4] & DO.NO_LANES))


def _everything(env):
    out = dict(state=env.get_state(), memory=env.policy_memory(), episodes=env.episodes(), counters=env.counters())
    out.update({"status_" + k: v for k, v in env.status().items()})
    return out


def _snapshots(env):
    env.restore(np.ones(env.n, dtype=bool))
    return env.get_state()


def _same(got, want, what):
    from pomcpp_amd.state import STATE_DTYPE
    if got.tobytes() != want.tobytes():
        for j in range(len(got)):
            for f in STATE_DTYPE.names:
                assert np.array_equal(got[j][f], want[j][f]), f"{what}: env {j}, {f}:\n{got[j][f]}\n{want[j][f]}"


@gpu
@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda v: "-".join(map(str, v)))
def test_layouts_start_all_then_next_under_a_mask(hip_lib, mixed_words, layout, offset):
    import torch
    if layout == MIXED:   # before any device call
        assert all(f >= 1 and a >= 1 and d >= 3 for words in mixed_words.values() for f, a, d in per_tile(words))
    g0, mask = start_games(), next_mask()
    want, want_words = DO.deal_many(SEED, np.arange(N), g0, layout, offset)
    if layout == MIXED:   # ... and on the boards this call deals
        assert all(f >= 1 and a >= 1 and d >= 3 for f, a, d in per_tile(want_words)), per_tile(want_words)
    env, _ = _handle(offset)
    with env:
        env.step_simple(2, 3)   # agents with a memory
        games = torch.from_numpy(g0.copy()).cuda()
        out = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
        env.deal(games, seed=SEED, layout=_layout(layout), out=out)
        words = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(words, want_words), np.flatnonzero(words != want_words)
        _same(env.get_state(), want, "START, ALL")
        g1 = DO.next_game(g0)
        assert np.array_equal(games.cpu().numpy(), g1) and (g1[g0 == 2 ** 31 - 1] == -2 ** 31).all()
        assert not env.policy_memory().any() and not env.status()["done"].any() and not env.status()["ubflags"].any()
        # NEXT under the mask: the records stay, the snapshots of the masked envs are their next boards, the others' the START boards
        before = _everything(env)
        out.fill_(SENTINEL)
        env.deal(games, seed=SEED, mode="next", which=torch.from_numpy(mask.astype(np.int32) * 3).cuda(), layout=_layout(layout), out=out)
        after = _everything(env)
        for k in before:
            assert np.asarray(after[k]).tobytes() == np.asarray(before[k]).tobytes(), k
        nxt, nxt_words = DO.deal_many(SEED, np.flatnonzero(mask), g1[mask], layout, offset)
        words = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(words[mask], nxt_words) and not words[~mask].any()
        assert np.array_equal(games.cpu().numpy(), np.where(mask, DO.next_game(g1), g1))
        snap = _snapshots(env)
        _same(snap[mask], nxt, "NEXT, MASK: the dealt envs' snapshots")
        _same(snap[~mask], want[~mask], "NEXT, MASK: the other envs' snapshots")


@gpu
def test_a_range_inside_tiles_and_the_invariants(hip_lib):
    """the mixed layout on first = 5, count = 37: everything outside the range is byte for byte as it was — States, snapshots, game
    counters, result words — and what is inside has what every dealt board has, by the independent search of tests/test_deal_host.py"""
    import torch
    first, count, offset = 5, 37, 2 ** 32 - 40
    inside = (np.arange(N) >= first) & (np.arange(N) < first + count)
    g0 = start_games()
    env, start = _handle(offset)
    with env:
        env.step_simple(2, 30)   # memories, finished envs, counters
        before = _everything(env)
        assert before["status_done"].any() and before["memory"].any()
        games = torch.from_numpy(g0.copy()).cuda()
        out = torch.full((N,), SENTINEL, dtype=torch.int32, device="cuda")
        env.deal(games, seed=SEED, first=first, count=count, layout=_layout(MIXED), out=out)
        after = _everything(env)
        want, want_words = DO.deal_many(SEED, np.flatnonzero(inside), g0[inside], MIXED, offset)
        for k in before:
            if k in ("episodes", "counters"):
                assert np.array_equal(after[k], before[k]), k
            else:
                assert after[k][~inside].tobytes() == before[k][~inside].tobytes(), k
        words = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(words[inside], want_words) and (words[~inside] == SENTINEL).all()
        _same(after["state"][inside], want, "the range")
        assert not after["memory"][inside].any() and not after["status_done"][inside].any() and not after["status_ubflags"][inside].any()
        assert np.array_equal(games.cpu().numpy(), np.where(inside, DO.next_game(g0), g0))
        fallback, attempts = check_invariants(after["state"][inside], words[inside], MIXED)
        assert fallback.any() and not fallback.all() and len(set(attempts.tolist())) >= 5
        snap = _snapshots(env)
        _same(snap[inside], want, "the range's snapshots")
        _same(snap[~inside], start[~inside], "the other snapshots")
