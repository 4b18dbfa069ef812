#!/usr/bin/env python3
"""Time pom_batch_deal (BatchEnvironment.deal) beside what it replaces and what it rides on.

  start      deal(START, ALL), the standard layout
  host way   the only way before it: the rule vectorised in numpy (below; checked here against tests/deal_oracle.py) plus make_game
             (the wrapper's name of pom_batch_upload: BatchEnvironment.upload is the same method)
  generate   pom_batch_generate: the cost of the old distribution
  next       deal(NEXT, RESTARTED) behind a step_mixed tick of SimpleAgent games --ticks ticks in, with the envs it dealt
  idle       the same call on a handle where nothing has restarted, beside the smallest launch torch makes (one element filled) timed the
             same way: what a pair of events around any single launch shows
  loop       the loop tick step_mixed + deal(NEXT, RESTARTED), beside step_mixed on a fresh_boards = 1 handle, which draws the old board
             inside the tick

Single calls — synchronise, one pair of HIP events around the call, synchronise — the sequences alternating in one run, the median of
--reps with their spread.  The host way is wall-clock time, --host-reps times.
usage (on the GPU box): python scripts/deal_bench.py [--envs N] [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
from pomcpp_amd.state import Item, new_states
from tests import deal_oracle as DO
from tests.imagine_oracle import below, board_draw, board_key

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=40, help="SimpleAgent ticks played before the loop measurements")
ap.add_argument("--reps", type=int, default=16)
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("deal_bench: no GPU — nothing is measured without one")
n, SEED = a.envs, 1
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)


def numpy_boards(seed, envs, games, layout=DO.STANDARD):
    """THE RULE on whole arrays: what a user with numpy would write.  Sequential where the rule is (40 pairs, the woods), vectorised over envs."""
    num_rigid, num_wood, num_items, max_bad, flags = layout
    L = DO.lane_woods(layout)
    m = len(envs)
    key = board_key(seed, envs, games)
    hi = np.array([y * 11 + x for (x, y), _ in DO.PAIRS])
    lo = np.array([y * 11 + x for _, (x, y) in DO.PAIRS])
    fixed_wood = np.zeros(121, dtype=bool)
    agents = np.zeros(121, dtype=bool)
    for (x, y), kind in DO.FIXED.items():
        fixed_wood[y * 11 + x] = kind == "lane" and L > 0
        agents[y * 11 + x] = kind.startswith("agent")
    rigid, wood = np.zeros((m, 121), dtype=bool), np.zeros((m, 121), dtype=bool)
    todo, bad, attempts = np.ones(m, dtype=bool), np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for att in range(DO.ATTEMPTS):
        idx = np.flatnonzero(todo)
        if idx.size == 0:
            break
        need_r, need_w = np.full(idx.size, num_rigid // 2), np.full(idx.size, (num_wood - L) // 2)
        r, w = np.zeros((idx.size, 121), dtype=bool), np.tile(fixed_wood, (idx.size, 1))
        for k in range(40):
            t = below(board_draw(key[idx], 64 * att + k), 40 - k).astype(np.int64)
            is_r = t < need_r
            is_w = ~is_r & (t < need_r + need_w)
            r[:, hi[k]] = r[:, lo[k]] = is_r
            w[:, hi[k]] = w[:, lo[k]] = is_w
            need_r, need_w = need_r - is_r, need_w - is_w
        open_ = ~r.reshape(-1, 11, 11)
        reach = np.zeros_like(open_)
        reach[:, 1, 1] = True
        while True:
            grown = reach.copy()
            grown[:, 1:] |= reach[:, :-1]
            grown[:, :-1] |= reach[:, 1:]
            grown[:, :, 1:] |= reach[:, :, :-1]
            grown[:, :, :-1] |= reach[:, :, 1:]
            grown &= open_
            if (grown == reach).all():
                break
            reach = grown
        b = (~r & ~w & ~agents & ~reach.reshape(-1, 121)).sum(1)
        rigid[idx], wood[idx], bad[idx], attempts[idx] = r, w, b, att + 1
        todo[idx] = b > max_bad
    left, need = wood.sum(1), np.full(m, num_items)
    flag = np.zeros((m, 121), dtype=np.int64)
    for c in range(121):
        chosen = wood[:, c] & (below(board_draw(key, 1024 + c), left).astype(np.int64) < need)
        flag[:, c] = np.where(chosen, 1 + below(board_draw(key, 1280 + c), 3).astype(np.int64), 0)
        need, left = need - chosen, left - wood[:, c]
    states = new_states(m)
    board = np.where(rigid, Item.RIGID, np.where(wood, Item.WOOD + flag, Item.PASSAGE))
    for i, (x, y) in enumerate(DO.AGENTS):
        board[:, y * 11 + x] = Item.AGENT0 + i
        states["agents"]["x"][:, i], states["agents"]["y"][:, i] = x, y
    states["board"] = board.reshape(m, 11, 11)
    words = DO.DEALT | np.where(todo, DO.FALLBACK, 0) | ((attempts - 1) << DO.ATTEMPTS_SHIFT) | (bad << DO.BAD_SHIFT)
    return states, words.astype(np.uint32)


def timed(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def row(name, ts, note=""):
    return f"{name:<34s} {statistics.median(ts):10.1f} {min(ts):10.1f} {max(ts):10.1f}  {note}"


# ---- the check, before anything is timed: the numpy twin against the literal checker, the call against the twin --------------------
k = 256
want, want_words = DO.deal_many(SEED, np.arange(k), np.arange(k) % 3)
twin, twin_words = numpy_boards(SEED, np.arange(k), np.arange(k) % 3)
if twin.tobytes() != want.tobytes() or not np.array_equal(twin_words, want_words):
    sys.exit("deal_bench: the numpy twin differs from the checker")
plain = BatchEnvironment(n, mode=MODE_ENV, stream=stream.cuda_stream)
plain.make_game(pa.make_boards(n, seed=1))
games, words = pa.new_games(n), torch.zeros((n,), dtype=torch.int32, device="cuda")
plain.deal(games, seed=SEED, out=words, stream=stream)
plain.sync()
twin, twin_words = numpy_boards(SEED, np.arange(n), np.zeros(n, dtype=np.int64))
if plain.get_state().tobytes() != twin.tobytes() or not np.array_equal(words.cpu().numpy().view(np.uint32), twin_words):
    sys.exit("deal_bench: the call differs from the rule in numpy")
att = ((twin_words >> 8) & 0xFF) + 1

# ---- the handles of the loop measurements ----------------------------------------------------------------------------------------
loop = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800, stream=stream.cuda_stream)
loop.make_game(pa.make_boards(n, seed=1))
loop_games, loop_words = pa.new_games(n), torch.zeros((n,), dtype=torch.int32, device="cuda")
loop.deal(loop_games, seed=SEED, stream=stream)
loop.deal(loop_games, seed=SEED, mode="next", stream=stream)
fresh = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800, fresh_boards=True, board_seed=SEED, stream=stream.cuda_stream)
fresh.generate(SEED)
idle = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800, stream=stream.cuda_stream)
idle.make_game(pa.make_boards(n, seed=1))
idle_games = pa.new_games(n)
for h in (loop, fresh, idle):
    h.step_mixed(0, 0, None, 15, SEED, 0, stream=stream)   # the agents' memory, allocated once
for t in range(a.ticks):
    loop.step_mixed(0, n, None, 15, SEED, t, stream=stream)
    loop.deal(loop_games, seed=SEED, mode="next", which="restarted", stream=stream)
    fresh.step_mixed(0, n, None, 15, SEED, t, stream=stream)
for h in (loop, fresh, idle, plain):
    h.sync()

T = {name: [] for name in ("start", "generate", "tick", "next", "idle", "empty", "loop", "fresh")}
dealt = []
tick = a.ticks
for rep in range(a.reps):
    T["start"].append(timed(lambda: plain.deal(games, seed=SEED, stream=stream)))
    T["generate"].append(timed(lambda: plain.generate(SEED + rep)))
    T["tick"].append(timed(lambda: loop.step_mixed(0, n, None, 15, SEED, tick, stream=stream)))
    T["next"].append(timed(lambda: loop.deal(loop_games, seed=SEED, mode="next", which="restarted", out=loop_words, stream=stream)))
    dealt.append(int((loop_words & 1).sum()))
    T["idle"].append(timed(lambda: idle.deal(idle_games, seed=SEED, mode="next", which="restarted", stream=stream)))
    T["empty"].append(timed(lambda: words[:1].zero_()))
    tick += 1

    def both():
        loop.step_mixed(0, n, None, 15, SEED, tick, stream=stream)
        loop.deal(loop_games, seed=SEED, mode="next", which="restarted", stream=stream)
    T["loop"].append(timed(both))
    T["fresh"].append(timed(lambda: fresh.step_mixed(0, n, None, 15, SEED, tick, stream=stream)))
    tick += 1
hs = []
for rep in range(a.host_reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    plain.make_game(numpy_boards(SEED, np.arange(n), np.full(n, rep + 1))[0])
    plain.sync()
    hs.append((time.perf_counter() - t0) * 1e3)

lines = [f"deal_bench: {n} envs, the standard layout {DO.STANDARD}; single calls, HIP events, median of {a.reps}, the sequences alternating in one run",
         f"the call equals the rule in numpy on all {n} envs ({att.mean():.3f} attempts a board, at most {att.max()}; no fallback: {not (twin_words & 2).any()})",
         f"{'':<34s} {'us: median':>10s} {'min':>10s} {'max':>10s}",
         row("deal(START, ALL)", T["start"], f"{n} envs dealt"),
         row("pom_batch_generate (old board)", T["generate"], f"{n} envs"),
         f"{'numpy + make_game (the way before)':<34s} {statistics.median(hs) * 1e3:10.0f} {min(hs) * 1e3:10.0f} {max(hs) * 1e3:10.0f}  "
         f"{statistics.median(hs) * 1e3 / statistics.median(T['start']):.0f} x the call",
         row("step_mixed tick, SimpleAgent x4", T["tick"], f"games {a.ticks}+ ticks in"),
         row("deal(NEXT, RESTARTED) behind it", T["next"], f"{min(dealt)} .. {max(dealt)} envs dealt a call"),
         row("deal(NEXT, RESTARTED), none restarted", T["idle"], "0 envs dealt"),
         row("a one-element torch fill", T["empty"], "the smallest launch, timed the same way"),
         row("loop tick: step_mixed + deal", T["loop"]),
         row("step_mixed, fresh_boards = 1", T["fresh"], "the old board drawn inside the tick")]
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
for h in (plain, loop, fresh, idle):
    h.close()
