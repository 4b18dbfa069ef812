#!/usr/bin/env python3
"""Time pom_batch_forecast (K = 1, 4, 12; idle and with first-tick moves) beside the launch it is modelled on: the resident
several-tick launch of a RAW handle, pom_batch_step_random(seed, POM_DIST_HARMLESS, K, ticks_per_launch = K), which plays the same
K ticks on the tile in LDS and additionally stores it.  HIP events around repeated calls, the paths alternating inside every
repetition, the median and the spread of the repetitions.

The two do not see the same boards for long: the forecast leaves the batch alone and meets the same mid-game states in every call;
the yardstick steps them, and under harmless moves (nobody plants) the boards fall quiet within a dozen ticks.  So the yardstick is
measured twice: `loop` as the calls follow each other (mostly quiet boards), and `fresh` with every env put back on the mid-game
states before each timed call (the boards the forecast sees; one call per pair of events, after a synchronisation: the figure also
holds the start of a single call from an idle device and the fork / join of the sub-streams).  The forecast is measured both ways
too: `idle` / `moves` as calls in a row, `single` like `fresh`, so that like stands beside like; and the cost per further tick
(K = 12 against K = 1) is set beside the yardstick's, which leaves the fixed parts out.
usage (on the GPU box): python scripts/forecast_bench.py [--envs N] [--reps R] [--calls C] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import DIST_HARMLESS, MODE_ENV, MODE_RAW, BatchEnvironment

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--reps", type=int, default=7, help="repetitions of the timed loop (the median is reported)")
ap.add_argument("--calls", type=int, default=200, help="calls per timed loop")
ap.add_argument("--fresh-calls", type=int, default=20, help="restore + one timed call, this many times per repetition")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("forecast_bench: no GPU — nothing is measured without one")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
n = a.envs
env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
env.step_simple(1, 150)
mid = env.get_state()
raw = BatchEnvironment(n, mode=MODE_RAW, stream=stream.cuda_stream)
raw.make_game(mid)  # (the upload is also the snapshot restore() goes back to)
everyone = np.ones(n, dtype=bool)
moves = torch.randint(0, 6, (n, 4), dtype=torch.int32, device="cuda")
out = env.forecast(1)

KS = (1, 4, 12)
paths = {}
for k in KS:
    paths[f"forecast K={k} idle"] = lambda k=k: env.forecast(k, out=out)
    paths[f"forecast K={k} moves"] = lambda k=k: env.forecast(k, moves=moves, out=out)
    paths[f"step_random K={k} loop"] = lambda k=k: raw.step_random(7, DIST_HARMLESS, ticks=k, ticks_per_launch=k)
for call in paths.values():  # warm-up: every shape the timed window uses
    for _ in range(5):
        call()
raw.sync()
torch.cuda.synchronize()
times = {name: [] for name in paths}
times.update({f"step_random K={k} fresh": [] for k in KS})
times.update({f"forecast K={k} single": [] for k in KS})
for rep in range(a.reps):  # the paths alternate inside a repetition: what disturbs one disturbs its neighbours too
    for name, call in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        raw.sync()  # (joins the yardstick's sub-streams: the events bracket whole calls)
        e0.record(stream)
        for _ in range(a.calls):
            call()
        raw.flush()
        e1.record(stream)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
    for k in KS:
        one = []
        for _ in range(a.fresh_calls):
            raw.restore(everyone)
            raw.sync()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            raw.step_random(7, DIST_HARMLESS, ticks=k, ticks_per_launch=k)
            raw.flush()
            e1.record(stream)
            torch.cuda.synchronize()
            one.append(e0.elapsed_time(e1) * 1e3)
        times[f"step_random K={k} fresh"].append(statistics.median(one))
        one = []
        for _ in range(a.fresh_calls):
            raw.sync()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            env.forecast(k, out=out)
            e1.record(stream)
            torch.cuda.synchronize()
            one.append(e0.elapsed_time(e1) * 1e3)
        times[f"forecast K={k} single"].append(statistics.median(one))
lines = [f"forecast_bench: {n} envs, mid-game ffa states (150 SimpleAgent ticks), {a.reps} repetitions of {a.calls} calls "
         f"(fresh: of {a.fresh_calls} single calls), us per call",
         f"{'path':32s} {'median':>8s} {'min':>8s} {'max':>8s}"]
med = {}
for name in sorted(times, key=lambda s: (int(s.split("K=")[1].split()[0]), s)):
    ts = times[name]
    med[name] = statistics.median(ts)
    lines.append(f"{name:32s} {med[name]:8.1f} {min(ts):8.1f} {max(ts):8.1f}")
for k in KS:
    f, y = med[f"forecast K={k} single"], med[f"step_random K={k} fresh"]
    lines.append(f"K={k}: single forecast / single yardstick call on the same boards = {f:.1f} / {y:.1f} = {f / y:.2f}"
                 f"{'' if f <= 1.25 * y else '  (more than a quarter above)'}")
span = KS[-1] - KS[0]
per = {w: (med[f"{w.split()[0]} K={KS[-1]} {w.split()[1]}"] - med[f"{w.split()[0]} K={KS[0]} {w.split()[1]}"]) / span
       for w in ("forecast idle", "forecast single", "step_random fresh", "step_random loop")}
lines.append(f"per further tick (K={KS[-1]} against K={KS[0]}): " + ", ".join(f"{w} {v:.1f}" for w, v in per.items()) + " us")
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
env.close()
raw.close()
