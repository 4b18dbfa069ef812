#!/usr/bin/env python3
"""bench.py --full's `throughput_T16_4096_envs` segment by itself: 4,096 envs, 16 ticks per launch (the tile stays in LDS between the
ticks, no hand-off), one wavefront per four SIMDs — a low-noise reading of what a wavefront's own tick costs.

    [POM_LIB=some/libpom_batch.so] python scripts/throughput_t16.py [--envs 4096] [--tpl 16] [--reps 5]

Same boards, move stream, warm-up (320 ticks) and timed length (40 launches) as the bench's segment; prints us per tick per repetition."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=4096)
ap.add_argument("--tpl", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--seed", type=int, default=1)
a = ap.parse_args()

import torch  # noqa: E402

import pomcpp_amd as pa  # noqa: E402
from pomcpp_amd.batch import MODE_ENV, BatchEnvironment  # noqa: E402

stream = torch.cuda.Stream(device=0)
torch.cuda.set_stream(stream)
env = BatchEnvironment(a.envs, device=0, mode=MODE_ENV, auto_reset=True, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(a.envs, seed=a.seed * 1000003, kind="ffa"))
launches = 40
env.step_random(a.seed, 1, ticks=320, ticks_per_launch=a.tpl)
env.sync()
out = []
for _ in range(a.reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    env.step_random(a.seed, 1, ticks=launches * a.tpl, ticks_per_launch=a.tpl)
    env.flush()
    e1.record(stream)
    env.sync()
    out.append(e0.elapsed_time(e1) / (launches * a.tpl) * 1e3)
env.close()
print(f"T{a.tpl} {a.envs} envs: " + " ".join(f"{v:.3f}" for v in out) + f" us per tick (median {sorted(out)[len(out) // 2]:.3f})")
