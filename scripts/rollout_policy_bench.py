#!/usr/bin/env python3
"""Time pom_batch_rollout_policy (K = 32, all four agents SimpleAgent, mid-game boards reached by step_simple) beside the way such
playouts were obtained before it existed: a second handle of n x R envs whose first n envs hold the roots (the upload is also their
snapshot), a device-side copy_envs fan-out of the roots' snapshots over all n x R envs (fresh agents), set_tick(0),
step_simple(seed, 32) and status().  The rollout is called with fresh_agents for the same reason.  In the same run, on the same
boards: pom_batch_rollout under POM_DIST_RANDOM, for the price of SimpleAgent against random play.

Shapes: 4,096 envs x 16 samples, 65,536 envs x 4, and the tree-search shape 256 envs x 256.  HIP events on the handles' stream
around ONE call (the rollouts) or one fan-out + step_simple + status (the fan-out way), each after a synchronisation, the paths
alternating inside every repetition; warm-up first; median, min and max of the repetitions, and the ratios of the medians.  The
fan-out way does not play the same samples (its env keys are those of the big handle), only the same amount of them on the same
boards; its statuses end in host memory, the rollout's words stay on the device.
usage (on the GPU box): python scripts/rollout_policy_bench.py [--reps R] [--out FILE]"""
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
ap.add_argument("--reps", type=int, default=16, help="timed repetitions per path and shape (the median is reported)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--pre-ticks", type=int, default=40, help="step_simple ticks that lead to the mid-game boards")
ap.add_argument("--shapes", default="4096x16,65536x4,256x256", help="envs x samples, comma-separated")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_policy_bench: no GPU — nothing is measured without one")
if a.reps < 16:
    sys.exit("rollout_policy_bench: at least 16 repetitions")
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


lines = [f"rollout_policy_bench: K = {K}, simple_mask 0xF, fresh agents, boards played {a.pre_ticks} ticks by step_simple; {a.reps} single "
         f"calls per path after {a.warmup} warm-up calls, the paths alternating; us per call (HIP events on the handles' stream)",
         f"{'shape':>14s} {'path':14s} {'median':>9s} {'min':>9s} {'max':>9s}      playouts/s   finished"]
missed = []
for shape in a.shapes.split(","):
    n, R = (int(v) for v in shape.split("x"))
    roots = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=MAX_STEPS, stream=stream.cuda_stream)
    roots.make_game(pa.make_boards(n, seed=1))
    roots.step_simple(3, a.pre_ticks)
    mid = roots.get_state()
    out = torch.empty((R, n), dtype=torch.int32, device="cuda")
    out_rnd = torch.empty((R, n), dtype=torch.int32, device="cuda")
    big = BatchEnvironment(n * R, mode=MODE_ENV, auto_reset=False, max_steps=MAX_STEPS, stream=stream.cuda_stream)
    big.make_game(mid)  # the first n envs and their snapshots; the others are overwritten by every fan-out
    src = (torch.arange(n * R, dtype=torch.int64, device="cuda") % n).contiguous()
    st = {}

    def policy():
        roots.rollout(K, R, SEED, DIST_RANDOM, out=out, simple=0xF, fresh_agents=True)

    def random():
        roots.rollout(K, R, SEED, DIST_RANDOM, out=out_rnd)

    def fanout():
        big.copy_envs(src, 0, from_snapshot=True)
        big.set_tick(0)
        big.step_simple(SEED, K)
        st.update(big.status())

    def sync():
        roots.sync()
        big.sync()

    paths = {"policy": policy, "fan-out": fanout, "random": random}
    for _ in range(a.warmup):
        for call in paths.values():
            call()
    sync()
    torch.cuda.synchronize()
    # like for like: the statuses the fan-out way reads are as far along as the rollout's words
    done = {"policy": float(((out & 0x10) != 0).float().mean()), "fan-out": float((st["done"] != 0).mean()),
            "random": float(((out_rnd & 0x10) != 0).float().mean())}
    t = {k: [] for k in paths}
    for rep in range(a.reps):
        for k, call in paths.items():
            t[k].append(timed(call, sync))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in paths:
        lines.append(f"{n:>8d}x{R:<5d} {k:14s} {med[k]:9.1f} {min(t[k]):9.1f} {max(t[k]):9.1f}   {n * R / med[k] * 1e6:13.3e}   "
                     f"{100 * done[k]:5.1f} % of the games finished within {K} ticks")
    slower = med["policy"] > med["fan-out"]
    if slower:
        missed.append(shape)
    lines.append(f"{n:>8d}x{R:<5d} policy / fan-out = {med['policy']:.1f} / {med['fan-out']:.1f} = {med['policy'] / med['fan-out']:.2f}"
                 f"{'  (the rollout is SLOWER)' if slower else ''};  policy / random = {med['policy']:.1f} / {med['random']:.1f} = "
                 f"{med['policy'] / med['random']:.2f}")
    del policy, random, fanout, sync, paths
    roots.close()
    big.close()
lines.append("the one-launch rollout's median is no longer than the fan-out way's at every shape" if not missed else
             "MISSED: the one-launch rollout's median is longer than the fan-out way's at " + ", ".join(missed))
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
