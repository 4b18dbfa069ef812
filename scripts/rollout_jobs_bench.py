#!/usr/bin/env python3
"""Time pom_batch_rollout_jobs (K = 32, mid-game boards reached by step_simple) beside the ways such playouts were obtained before
it existed, every baseline made of calls that exist without it and timed in the same run, on the same boards:

  (a) move table   65,536 envs x 6 moves x 4 samples of agent 0.  New: ONE move_table call (6 n jobs).  Old: six
                   rollout(..., moves=, first=[0]) calls and the torch.stack of their results.  With random opponents (simple = 0)
                   and with the other three agents playing SimpleAgent (simple = 0xE).
  (b) leaf subset  8,192 sources drawn at random (with repeats, in no order) from 65,536 envs, 16 samples, all four agents
                   SimpleAgent.  New: ONE rollout_jobs call.  Old 1: a whole-batch rollout and index_select of the 8,192 columns.
                   Old 2: a second handle of 8,192 envs that already holds the sources' states, and rollout there.  Getting the
                   leaves into it is NOT timed (copy_envs copies inside one handle, so across two they go through the host): this
                   is a floor under every two-handle way.  Its draws are keyed by its own env numbers and its agents are fresh: the
                   same amount of playouts, not the same samples.
                   The comparison is against the faster of the two.
  (c) identity     65,536 envs x 4 samples with src = arange(n): the same words as rollout with the same arguments, which is the
                   baseline — the price of the list where nothing is gained from it (random and 0xF).

HIP events on the handles' stream around ONE call (or one old-way sequence), each after a synchronisation, the paths of a comparison
alternating inside every repetition; warm-up first; median, min and max of the repetitions.  A new way counts as faster only where
its median lies below the old way's by more than the old way's own spread (max - min of its repetitions).
usage (on the GPU box): python scripts/rollout_jobs_bench.py [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import DIST_RANDOM, MODE_ENV, BatchEnvironment

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=16, help="timed repetitions per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--pre-ticks", type=int, default=40, help="step_simple ticks that lead to the mid-game boards")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--leaves", type=int, default=8192)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_jobs_bench: no GPU — nothing is measured without one")
if a.reps < 16:
    sys.exit("rollout_jobs_bench: at least 16 repetitions")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
K, MAX_STEPS, SEED, n, m = a.horizon, 800, 7, a.envs, a.leaves
dev = torch.device("cuda")

roots = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=MAX_STEPS, stream=stream.cuda_stream)
roots.make_game(pa.make_boards(n, seed=1))
roots.step_simple(3, a.pre_ticks)
small = BatchEnvironment(m, mode=MODE_ENV, auto_reset=False, max_steps=MAX_STEPS, stream=stream.cuda_stream)
small.make_game(pa.make_boards(m, seed=2))   # (b) puts the leaves there
handles = [roots, small]


def sync():
    for h in handles:
        h.sync()
    torch.cuda.synchronize()


def timed(call):
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def compare(title, playouts, paths, new, old, check=None):
    """paths: name -> call, timed alternating; `new` against the fastest of `old`"""
    for _ in range(a.warmup):
        for call in paths.values():
            call()
    sync()
    if check:
        check()
    t = {k: [] for k in paths}
    for _ in range(a.reps):
        for k, call in paths.items():
            t[k].append(timed(call))
    med = {k: statistics.median(v) for k, v in t.items()}
    lines.append(title)
    for k in paths:
        lines.append(f"    {k:34s} {med[k]:10.1f} {min(t[k]):10.1f} {max(t[k]):10.1f} {max(t[k]) - min(t[k]):9.1f}   {playouts / med[k] * 1e6:11.3e}")
    best = min(old, key=lambda k: med[k])
    spread = max(t[best]) - min(t[best])
    gain = med[best] - med[new]
    verdict = "FASTER by more than that spread" if gain > spread else "NOT faster by more than that spread" if gain > 0 else "SLOWER"
    lines.append(f"    {new} / {best} = {med[new]:.1f} / {med[best]:.1f} = {med[new] / med[best]:.3f}; the old way's spread {spread:.1f} us: "
                 f"the new call is {verdict}")
    return gain > spread


lines = [f"rollout_jobs_bench: K = {K}, {n} envs played {a.pre_ticks} ticks by step_simple; {a.reps} single calls per path after {a.warmup} "
         f"warm-up calls, each after a synchronisation, the paths of a comparison alternating; us per call (HIP events on the handles' stream)",
         f"    {'path':34s} {'median':>10s} {'min':>10s} {'max':>10s} {'max-min':>9s}    playouts/s"]
verdicts = {}

# ---- (a) the move table --------------------------------------------------------------------------------------------------------
R = 4
six_moves = []
for c in range(6):
    mv = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    mv[:, 0] = c
    six_moves.append(mv)
six_out = [torch.empty((R, n), dtype=torch.int32, device=dev) for _ in range(6)]
res = {}
for simple, who in ((0, "random opponents"), (0xE, "the other three SimpleAgent")):
    def table(simple=simple):
        res["new"] = roots.move_table(0, K, R, SEED, DIST_RANDOM, simple=simple)

    def six(simple=simple):
        for c in range(6):
            roots.rollout(K, R, SEED, DIST_RANDOM, moves=six_moves[c], out=six_out[c], simple=simple, first=[0])
        res["old"] = torch.stack(six_out)

    def same():
        assert torch.equal(res["new"], res["old"]), "the move table is not the six calls' words"

    verdicts[f"(a) {who}"] = compare(f"(a) move table, {n} envs x 6 moves x {R} samples, {who}", 6 * n * R,
                                     {"move_table (one call)": table, "six rollout calls + stack": six}, "move_table (one call)",
                                     ["six rollout calls + stack"], same)
del six_moves, six_out
res.clear()

# ---- (b) a subset of leaves ----------------------------------------------------------------------------------------------------
R = 16
src = torch.randint(0, n, (m,), dtype=torch.int64, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
out_jobs = torch.empty((R, m), dtype=torch.int32, device=dev)
out_whole = torch.empty((R, n), dtype=torch.int32, device=dev)
out_small = torch.empty((R, m), dtype=torch.int32, device=dev)


def jobs():
    roots.rollout_jobs(src, K, R, SEED, DIST_RANDOM, out=out_jobs, simple=0xF)


def whole():
    roots.rollout(K, R, SEED, DIST_RANDOM, out=out_whole, simple=0xF)
    res["whole"] = out_whole.index_select(1, src)


small.upload(roots.get_state()[src.cpu().numpy()])   # once, untimed (copy_envs copies within one handle: across two, through the host)


def second():
    small.rollout(K, R, SEED, DIST_RANDOM, out=out_small, simple=0xF, fresh_agents=True)


def same_b():
    assert torch.equal(out_jobs, res["whole"]), "the jobs' words are not the whole batch's, indexed by source"


verdicts["(b)"] = compare(f"(b) leaf subset, {m} sources out of {n} envs x {R} samples, simple 0xF", m * R,
                          {"rollout_jobs (one call)": jobs, "whole-batch rollout + index_select": whole,
                           "second handle, leaves in place": second},
                          "rollout_jobs (one call)", ["whole-batch rollout + index_select", "second handle, leaves in place"], same_b)

# ---- (c) the identity list -----------------------------------------------------------------------------------------------------
R = 4
ident = torch.arange(n, dtype=torch.int64, device=dev)
out_a = torch.empty((R, n), dtype=torch.int32, device=dev)
out_b = torch.empty((R, n), dtype=torch.int32, device=dev)
for simple, who in ((0, "random"), (0xF, "simple 0xF")):
    def new(simple=simple):
        roots.rollout_jobs(ident, K, R, SEED, DIST_RANDOM, out=out_a, simple=simple)

    def old(simple=simple):
        roots.rollout(K, R, SEED, DIST_RANDOM, out=out_b, simple=simple)

    def same_c():
        assert torch.equal(out_a, out_b), "an identity list does not give the rollout's words"

    compare(f"(c) identity list, {n} envs x {R} samples, {who} (the ratio is reported, no verdict is expected)", n * R,
            {"rollout_jobs, src = arange(n)": new, "rollout": old}, "rollout_jobs, src = arange(n)", ["rollout"], same_c)

missed = [k for k, ok in verdicts.items() if not ok]
lines.append("(a) and (b): the new call is faster than the old way by more than the old way's spread in every comparison" if not missed else
             "MISSED: not faster than the old way by more than its spread in " + ", ".join(missed))
text = "\n".join(lines)
print(text, flush=True)
for h in handles:
    h.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
