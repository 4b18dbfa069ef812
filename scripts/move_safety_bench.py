#!/usr/bin/env python3
"""Time pom_batch_move_safety (K = 1, 4, 12; agent masks 0x1 and 0xF; death_tick alone and with escape_tick) beside what it replaces:
the six-forecast recipe of INTEGRATION.md §B, six pom_batch_forecast calls with first-tick moves per agent (6 or 24 calls), which
give death_tick.  The recipe's move tensors are built before the clock starts, and its calls ask for agent_tick (the recipe's answer)
beside the flame plane the forecast always writes.

Single calls, as a search or a learner's action mask issues them: synchronise, one pair of HIP events around the call (or around the
recipe's 6 / 24 calls), synchronise; the paths alternate inside every repetition and the median of the repetitions is reported with
their spread.  The figures hold the start of a call from an idle device.
usage (on the GPU box): python scripts/move_safety_bench.py [--envs N] [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import MODE_ENV, BatchEnvironment

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=40, help="SimpleAgent ticks played before the measurement")
ap.add_argument("--reps", type=int, default=16, help="single calls per path (the median is reported)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("move_safety_bench: no GPU — nothing is measured without one")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
n = a.envs
env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
env.step_simple(1, a.ticks)
base = torch.randint(0, 6, (n, 4), dtype=torch.int32, device="cuda")
recipe_moves = {}
for agent in range(4):
    for m in range(6):
        mv = base.clone()
        mv[:, agent] = m
        recipe_moves[agent, m] = mv
out = env.move_safety(1, moves=base)
fc_out = env.forecast(1, moves=base)

KS = (1, 4, 12)
MASKS = ((0x1, (0,)), (0xF, (0, 1, 2, 3)))


def recipe(k, agents):
    for agent in agents:
        for m in range(6):
            env.forecast(k, moves=recipe_moves[agent, m], out=fc_out)


paths = {}
for k in KS:
    for mask, agents in MASKS:
        paths[f"K={k} mask {mask:#x} move_safety death"] = lambda k=k, mask=mask: env.move_safety(k, agents=mask, moves=base, out=out, escape=False)
        paths[f"K={k} mask {mask:#x} move_safety death+escape"] = lambda k=k, mask=mask: env.move_safety(k, agents=mask, moves=base, out=out)
        paths[f"K={k} mask {mask:#x} recipe: {6 * len(agents)} forecasts"] = lambda k=k, agents=agents: recipe(k, agents)
for call in paths.values():  # warm-up: every shape the timed window uses
    for _ in range(3):
        call()
env.sync()
torch.cuda.synchronize()
times = {name: [] for name in paths}
for rep in range(a.reps):  # the paths alternate inside a repetition: what disturbs one disturbs its neighbours too
    for name, call in paths.items():
        env.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)

env.move_safety(12, moves=base, out=out)  # what the boards are like: the BOMB column at K = 12
d = out["death_tick"].to(torch.int32)
x = out["escape_tick"].to(torch.int32)
lines = [f"move_safety_bench: {n} envs, ffa boards after {a.ticks} SimpleAgent ticks, base moves random, {a.reps} single calls per path, us per call "
         f"(recipe: per 6 / 24 calls)",
         f"at K=12, of {int((d[:, :, 5] >= 0).sum())} live agents' BOMB candidates {int((d[:, :, 5] > 0).sum())} die standing still and "
         f"{int((x[:, :, 5] > 0).sum())} have no way out",
         f"{'path':48s} {'median':>9s} {'min':>9s} {'max':>9s}"]
med = {}
for name, ts in times.items():
    med[name] = statistics.median(ts)
    lines.append(f"{name:48s} {med[name]:9.1f} {min(ts):9.1f} {max(ts):9.1f}")
for k in KS:
    for mask, agents in MASKS:
        r = med[f"K={k} mask {mask:#x} recipe: {6 * len(agents)} forecasts"]
        dd, de = med[f"K={k} mask {mask:#x} move_safety death"], med[f"K={k} mask {mask:#x} move_safety death+escape"]
        lines.append(f"K={k} mask {mask:#x}: death alone / recipe = {dd:.1f} / {r:.1f} = {dd / r:.2f}; with escape / recipe = {de:.1f} / {r:.1f} = {de / r:.2f}")
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
env.close()
