#!/usr/bin/env python3
"""Time pom_batch_rollout (K = 32, POM_DIST_RANDOM, mid-game boards) beside the way the same env-samples were obtained before it
existed: a second handle of n x R envs whose first n envs hold the roots (the upload is also their snapshot), a device-side
copy_envs fan-out of the roots' snapshots over all n x R envs, set_tick(0), step_random(seed, POM_DIST_RANDOM, 32, 1), and an
observation that carries env_attrs (the compact code planes, the cheapest one there is: the export cannot leave its planes out).

Shapes: 4,096 envs x 16 samples, 65,536 envs x 4, and the tree-search shape 256 envs x 256.  HIP events on the handles' stream
around ONE call (rollout) or one fan-out + step + observe (baseline), each after a synchronisation, the two alternating inside
every repetition; warm-up first; median, min and max of the repetitions, and the ratio of the medians.  The two do not play the
same samples (the baseline's env keys are those of the big handle), only the same amount of them on the same boards.
usage (on the GPU box): python scripts/rollout_bench.py [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import DIST_RANDOM, MODE_ENV, BatchEnvironment, _check

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=16, help="timed repetitions per path and shape (the median is reported)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--shapes", default="4096x16,65536x4,256x256", help="envs x samples, comma-separated")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_bench: no GPU — nothing is measured without one")
if a.reps < 16:
    sys.exit("rollout_bench: at least 16 repetitions")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
K, MAX_STEPS, SEED = a.horizon, 800, 7


def timed(call, sync):
    sync()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


lines = [f"rollout_bench: K = {K}, POM_DIST_RANDOM, boards played 57 ticks under POM_DIST_RANDOM; {a.reps} single calls per path after "
         f"{a.warmup} warm-up calls, the paths alternating; us per call (HIP events on the handles' stream)",
         f"{'shape':>14s} {'path':10s} {'median':>9s} {'min':>9s} {'max':>9s}   env-samples/s   finished"]
ratios = []
for shape in a.shapes.split(","):
    n, R = (int(v) for v in shape.split("x"))
    roots = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=MAX_STEPS, stream=stream.cuda_stream)
    roots.make_game(pa.make_boards(n, seed=1))
    roots.step_random(3, DIST_RANDOM, 57, 1)
    mid = roots.get_state()
    out = torch.empty((R, n), dtype=torch.int32, device="cuda")
    big = BatchEnvironment(n * R, mode=MODE_ENV, auto_reset=False, max_steps=MAX_STEPS, stream=stream.cuda_stream)
    big.make_game(mid)  # the first n envs and their snapshots; the others are overwritten by every fan-out
    src = (torch.arange(n * R, dtype=torch.int64, device="cuda") % n).contiguous()
    codes = torch.empty((n * R, 5, 11, 11), dtype=torch.uint8, device="cuda")
    env_attrs = torch.empty((n * R, 4), dtype=torch.int32, device="cuda")

    def rollout():
        roots.rollout(K, R, SEED, DIST_RANDOM, out=out)

    def baseline():
        big.copy_envs(src, 0, from_snapshot=True)
        big.set_tick(0)
        big.step_random(SEED, DIST_RANDOM, K, 1)
        _check(big._lib, big._lib.pom_batch_observe(big._h, codes.data_ptr(), 3, 0, None, env_attrs.data_ptr()))  # POM_OBS_CODES, env_attrs only

    def sync():
        roots.sync()
        big.sync()

    for _ in range(a.warmup):
        rollout()
        baseline()
    sync()
    torch.cuda.synchronize()
    # like for like: the statuses the baseline reads are as far along as the rollout's words
    done_r = float(((out & 0x10) != 0).float().mean())
    done_b = float(((env_attrs[:, 2] & 1) != 0).float().mean())
    t = {"rollout": [], "baseline": []}
    for rep in range(a.reps):
        t["rollout"].append(timed(rollout, sync))
        t["baseline"].append(timed(baseline, sync))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, frac in (("rollout", done_r), ("baseline", done_b)):
        lines.append(f"{n:>8d}x{R:<5d} {k:10s} {med[k]:9.1f} {min(t[k]):9.1f} {max(t[k]):9.1f}   {n * R / med[k] * 1e6:13.3e}   "
                     f"{100 * frac:5.1f} % of the games finished within {K} ticks")
    ratios.append((shape, med["rollout"] / med["baseline"]))
    lines.append(f"{n:>8d}x{R:<5d} rollout / baseline = {med['rollout']:.1f} / {med['baseline']:.1f} = {ratios[-1][1]:.2f}"
                 f"{'  (the rollout is SLOWER)' if ratios[-1][1] > 1 else ''}")
    del rollout, baseline, sync
    roots.close()
    big.close()
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
