#!/usr/bin/env python3
"""Time pom_batch_expand beside the way children were made before it existed, in the same run, on the same boards: on 65,536 envs
(mid-game boards reached by step_simple) 4,096 and 32,768 children of parents scattered over the lower half (drawn at random, with
repeats, in no order) are put into a tile-aligned range of the upper half.

  new   ONE expand call: copy, tick, result words (and, where said, the code-plane observation of the new nodes).
  old   copy_envs (device list: gather + scatter kernels) followed by step_device_range on that range (which writes the same
        observation where said): three launches.  The old way NEEDS the range to be whole tiles; expand does not.  It gives no
        result words: a status read-back would come on top and is not timed.

Both leave the same children (checked once per size).  HIP events on the handle's stream around ONE call (or one old-way sequence),
each after a synchronisation, the two paths alternating inside every repetition; warm-up first; median, min and max of the
repetitions.  No ratio is expected: the numbers are reported as they come.
usage (on the GPU box): python scripts/expand_bench.py [--reps R] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=16, help="timed repetitions per path (the median is reported)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--pre-ticks", type=int, default=40, help="step_simple ticks that lead to the mid-game boards")
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--children", type=int, nargs="+", default=[4096, 32768])
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("expand_bench: no GPU — nothing is measured without one")
if a.reps < 16:
    sys.exit("expand_bench: at least 16 repetitions")
n, half = a.envs, a.envs // 2
if half % 16 or any(m <= 0 or m % 16 or m > half for m in a.children):
    sys.exit("expand_bench: the old way needs whole tiles — envs / 2 and the children counts must be multiples of 16, children <= envs / 2")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
dev = torch.device("cuda")

env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=False, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
env.step_simple(3, a.pre_ticks)
codes = torch.zeros((n, 5, 11, 11), dtype=torch.uint8, device=dev)


def sync():
    env.sync()
    torch.cuda.synchronize()


def timed(call):
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


lines = [f"expand_bench: {n} envs played {a.pre_ticks} ticks by step_simple; parents drawn at random from envs 0..{half - 1}, children in the range "
         f"starting at env {half}; {a.reps} single calls per path after {a.warmup} warm-up calls, each after a synchronisation, the two paths "
         f"alternating; us per call (HIP events on the handle's stream)",
         f"    {'path':50s} {'median':>9s} {'min':>9s} {'max':>9s} {'max-min':>8s}   children/s"]
for m in a.children:
    gen = torch.Generator(device=dev).manual_seed(5 + m)
    src = torch.randint(0, half, (m,), dtype=torch.int64, device=dev, generator=gen)
    moves = torch.randint(0, 6, (m, 4), dtype=torch.int32, device=dev, generator=gen)
    full = torch.zeros((n, 4), dtype=torch.int32, device=dev)   # the old way's moves are indexed by env
    full[half:half + m] = moves
    words = torch.empty((m,), dtype=torch.int32, device=dev)
    for observe in (False, True):
        def new(observe=observe):
            env.expand(src, moves, first=half, out=words, codes=codes if observe else None, attrs=False)

        def old(observe=observe):
            env.copy_envs(src, first=half)
            env.step_device_range(half, m, full, codes=codes if observe else None)

        paths = {"expand (one launch)": new, "copy_envs + step_device_range (three launches)": old}
        for _ in range(a.warmup):
            for call in paths.values():
                call()
        # the same children either way
        new()
        sync()
        got, got_codes = env.get_state(half, m).tobytes(), codes[half:half + m].clone()
        old()
        sync()
        assert env.get_state(half, m).tobytes() == got, "expand's children are not the old way's"
        assert not observe or torch.equal(codes[half:half + m], got_codes), "expand's observation is not the old way's"
        t = {k: [] for k in paths}
        for _ in range(a.reps):
            for k, call in paths.items():
                t[k].append(timed(call))
        med = {k: statistics.median(v) for k, v in t.items()}
        lines.append(f"{m} children, {'with' if observe else 'without'} the code-plane observation")
        for k in paths:
            lines.append(f"    {k:50s} {med[k]:9.1f} {min(t[k]):9.1f} {max(t[k]):9.1f} {max(t[k]) - min(t[k]):8.1f}   {m / med[k] * 1e6:10.3e}")
        k_new, k_old = list(paths)
        spread = max(t[k_old]) - min(t[k_old])
        gain = med[k_old] - med[k_new]
        verdict = "FASTER by more than that spread" if gain > spread else "NOT faster by more than that spread" if gain > 0 else "SLOWER"
        lines.append(f"    expand / old = {med[k_new]:.1f} / {med[k_old]:.1f} = {med[k_new] / med[k_old]:.3f}; the old way's spread {spread:.1f} us: "
                     f"expand is {verdict}")
text = "\n".join(lines)
print(text, flush=True)
env.close()
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
