"""The corpus of tests/queue_first_trip_cases.py through the kernels: 32 envs (two tiles), every entry in turn in every column of a
tile while the other columns hold entries from the rest of the corpus (the pattern of tests/tile_mates.py) — a first trip taken with
another lane's slot, or a loop behind it entered for the wrong env, shows as an env that leaves its solo trace.

An env's expected State after tick t is its entry's SOLO run of the oracle (queue_first_trip_cases.traces), whatever its place:
all 1004 bytes, the flags gathered since upload, and at the end the step and flagged-tick counters.  Through the plain one-tick
launch (every tick) and through chained launches, calls of 3 and of 7 ticks; each batch is played again with a first call of 1 and
of 2 ticks (of 1 tick) in front, so that the state after every tick is looked at behind a call of each length."""
import numpy as np
import pytest

from tests import queue_first_trip_cases as QC
from tests.test_queue_first_trip import Stage

T = QC.TICKS
N = 32       # two tiles
STRIDE = 7   # neighbouring columns hold entries this far apart in the corpus: flame and bomb entries share every tile


@pytest.fixture(scope="module")
def stage(oracle):
    return Stage(oracle)


def placements(n_entries):
    """who[k][e]: the entry of env e in batch k.  Tile j of batch k holds entry 2k + j (mod E) in column 0, and the entries STRIDE
    further on per column: over the batches every entry comes to stand in every column"""
    batches = (n_entries + 1) // 2
    return [np.array([(2 * k + e // 16 + STRIDE * (e % 16)) % n_entries for e in range(N)], dtype=np.int64) for k in range(batches)]


def test_every_entry_stands_in_every_column(stage):
    E = len(stage.entries)
    seen = set()
    for who in placements(E):
        assert who.size == N
        for e, i in enumerate(who):
            seen.add((int(i), e % 16))
        for tile in (who[:16], who[16:]):
            kinds = {stage.names[i][:3] for i in tile}
            assert kinds == {"fl_", "bo_"}, kinds  # both kinds of queue busy in every tile
    assert seen == {(i, c) for i in range(E) for c in range(16)}


def _batch(stage, who):
    start = np.concatenate([stage.entries[i].start for i in who])
    moves = np.ascontiguousarray(np.stack([stage.entries[i].moves for i in who], axis=1).astype(np.int32))
    return start, moves


def _check(stage, who, t, env, what):
    got = env.get_state().view(np.uint8).reshape(N, 1004)
    ubs = np.asarray(env.status()["ubflags"], dtype=np.uint32)
    want = stage.states[who, t]
    bad = np.nonzero((got != want).any(axis=1) | (ubs != stage.sticky[who, t]))[0]
    if bad.size:
        k = int(bad[0])
        tile = [stage.names[i] for i in who[k - k % 16:k - k % 16 + 16]]
        raise AssertionError(f"{what}: env {k} (tile {k // 16}, column {k % 16}) entry {stage.names[who[k]]} tick {t}: bytes "
                             f"{np.nonzero(got[k] != want[k])[0][:12].tolist()} differ, ubflags {int(ubs[k]):#x} want "
                             f"{int(stage.sticky[who[k], t]):#x}; {bad.size} envs differ in all; its tile: {tile}")


def _check_counters(stage, who, env, before, what):
    """the counters grew by one game of the batch since `before`; returns them"""
    from pomcpp_amd.batch import CNT_EPISODES, CNT_RESETS, CNT_STEPS, CNT_UB_TICKS
    now = env.counters()
    cnt = now - before
    assert cnt[CNT_STEPS] == N * T and cnt[CNT_UB_TICKS] == int((stage.ubs[who] != 0).sum()), (what, cnt.tolist())
    assert cnt[CNT_EPISODES] == 0 and cnt[CNT_RESETS] == 0, (what, cnt.tolist())
    return now


@pytest.mark.gpu
def test_corpus_gpu_plain_launches_every_column_every_tick(hip_lib, stage):
    from pomcpp_amd.batch import MODE_RAW, BatchEnvironment
    with BatchEnvironment(N, mode=MODE_RAW) as env:  # one handle: an upload starts the next batch (status and flags clear)
        assert env.launch_shape()[:2] == (16, 4)
        cnt = env.counters()
        for k, who in enumerate(placements(len(stage.entries))):
            start, moves = _batch(stage, who)
            env.make_game(start)
            for t in range(T):
                env.step(moves[t])
                _check(stage, who, t, env, f"plain launch, batch {k}")
            cnt = _check_counters(stage, who, env, cnt, f"plain launch, batch {k}")


@pytest.mark.gpu
@pytest.mark.parametrize("piece", [3, 7])
def test_corpus_gpu_chained_launches_every_column(hip_lib, stage, piece):
    import torch
    from pomcpp_amd.batch import ISSUE_CHAIN, MODE_RAW, BatchEnvironment
    with BatchEnvironment(N, mode=MODE_RAW, issue_mode=ISSUE_CHAIN) as env:
        cnt = env.counters()
        for k, who in enumerate(placements(len(stage.entries))):
            start, moves = _batch(stage, who)
            dev_moves = torch.from_numpy(moves).to("cuda:0")
            for lead in range(min(piece, T - piece + 1)):
                pieces = ([lead] if lead else []) + [piece] * ((T - lead) // piece)
                pieces += [T - sum(pieces)] if sum(pieces) < T else []
                env.make_game(start)
                t = 0
                for n_ticks in pieces:
                    env.step_device_many(dev_moves[t:t + n_ticks].contiguous())
                    env.sync()
                    t += n_ticks
                    _check(stage, who, t - 1, env, f"chained calls {pieces}, batch {k}")
                assert t == T
                cnt = _check_counters(stage, who, env, cnt, f"chained calls {pieces}, batch {k}")
        stats = env.chain_stats()
        assert stats["tiles_recovered"] == 0 and stats["ticks_replayed"] == 0, stats  # every tile played every tick in its chained launch
