#!/usr/bin/env python3
"""Time the fogged per-agent views (pom_batch_observe_view and the fused step) beside the unfogged paths they stand next to, on
mid-game states: HIP events around repeated calls, the paths alternating inside every repetition, the median and the spread of the
repetitions.
usage (on the GPU box): python scripts/view_bench.py [--envs N] [--reps R] [--calls C] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--reps", type=int, default=7, help="repetitions of the timed loop (the median is reported)")
ap.add_argument("--calls", type=int, default=1000, help="calls per timed loop")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("view_bench: no GPU — nothing is measured without one")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
n = a.envs
env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
env.step_simple(1, 150)
moves = torch.randint(0, 6, (n, 4), dtype=torch.int32, device="cuda")

# name -> (what observe() is asked for, fused with a step?, bytes of planes written per env)
paths = {
    "a observe per_agent uint8": (dict(per_agent=True, dtype="uint8"), False, 7744),
    "b observe codes": (dict(dtype="codes"), False, 605),
    "c observe codes view_radius=4": (dict(dtype="codes", view_radius=4), False, 2420),
    "d observe uint8 view_radius=4": (dict(dtype="uint8", view_radius=4), False, 7744),
    "e1 step+observe per_agent uint8": (dict(per_agent=True, dtype="uint8"), True, 7744),
    "e2 step+observe codes view_radius=4": (dict(dtype="codes", view_radius=4), True, 2420),
}
outs = {}
for name, (kw, fused, _) in paths.items():  # warm-up: every shape the timed window uses
    call = (lambda out=None, kw=kw: env.step_device_observe(moves, out=out, **kw)) if fused else (lambda out=None, kw=kw: env.observe(out=out, **kw))
    outs[name] = call()[0]
    for _ in range(5):
        call(outs[name])
    paths[name] = (call, fused, paths[name][2])
torch.cuda.synchronize()
times = {name: [] for name in paths}
for rep in range(a.reps):  # the paths alternate inside a repetition: what disturbs one disturbs its neighbours too
    for name, (call, _, _) in paths.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(a.calls):
            call(outs[name])
        e1.record(stream)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) / a.calls * 1e3)
lines = [f"view_bench: {n} envs, mid-game ffa states (150 SimpleAgent ticks), {a.reps} repetitions of {a.calls} calls, us per call",
         f"{'path':40s} {'median':>8s} {'min':>8s} {'max':>8s}  planes B/env"]
med = {}
for name, ts in times.items():
    med[name] = statistics.median(ts)
    lines.append(f"{name:40s} {med[name]:8.1f} {min(ts):8.1f} {max(ts):8.1f}  {paths[name][2]}")
spread_a = max(times["a observe per_agent uint8"]) - min(times["a observe per_agent uint8"])
A, C_, D = med["a observe per_agent uint8"], med["c observe codes view_radius=4"], med["d observe uint8 view_radius=4"]
E1, E2 = med["e1 step+observe per_agent uint8"], med["e2 step+observe codes view_radius=4"]
lines.append(f"c <= a: {C_:.1f} <= {A:.1f}: {'met' if C_ <= A else 'MISSED'}")
lines.append(f"fused view-codes <= fused per-agent uint8: {E2:.1f} <= {E1:.1f}: {'met' if E2 <= E1 else 'MISSED'}")
lines.append(f"d <= a + spread of a ({spread_a:.1f}): {D:.1f} <= {A + spread_a:.1f}: {'met' if D <= A + spread_a else 'MISSED'}")
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
env.close()
