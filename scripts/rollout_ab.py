#!/usr/bin/env python3
"""A/B of the two entry points' kernels when no agent plays SimpleAgent: pom_batch_rollout (`rollout`), the same call a second time
(`rollout_again`, an A/A pair that shows the run's own noise) and pom_batch_rollout_policy with simple_mask 0 (`policy0`), the three
alternating inside every repetition.  Boards, shapes and timing as scripts/rollout_bench.py: make_boards(n, seed=1) played 57 ticks
under POM_DIST_RANDOM, max_steps 800; 4,096 envs x 16 samples, 65,536 x 4 and 256 x 256; K = 32; HIP events on the handle's stream
around ONE call after a synchronisation; warm-up first; median, min and max.  Every shape once without moves and once with a moves
tensor (tick 1 fixed for all four agents: first_mask 0xF).

The noise of a row is |median(rollout_again) / median(rollout) - 1|; policy0 QUALIFIES at a row when median(policy0) / median(rollout)
- 1 is at most twice that noise (the A/A pair is one draw of the noise only), and at once when it is faster.

This script decided whether the two kernels could be folded into one (profiles/rollout_one_kernel_ab.txt): policy0 did not qualify,
a folded kernel with pom_rollout_kernel's register-resident bookkeeping in its instance without the policy did not match
pom_rollout_kernel either, and the two kernels stayed.  Run on a library in which `rollout` and `policy0` are one kernel it is an
A/A/A check, and a row that does not qualify shows noise the A/A pair missed, nothing else.
usage (on the GPU box): python scripts/rollout_ab.py [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import DIST_RANDOM, MODE_ENV, BatchEnvironment

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=16, help="timed repetitions per path and row (the median is reported)")
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--horizon", type=int, default=32)
ap.add_argument("--shapes", default="4096x16,65536x4,256x256", help="envs x samples, comma-separated")
ap.add_argument("--commit", default=None, help="the commit the library was built at (default: git rev-parse HEAD, if there is a git)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("rollout_ab: no GPU — nothing is measured without one")
if a.reps < 16:
    sys.exit("rollout_ab: at least 16 repetitions")
commit = a.commit
if commit is None:
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
    commit = r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
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


lines = [f"rollout_ab: commit {commit}, library {os.path.basename(os.environ.get('POM_LIB', 'default'))}; K = {K}, POM_DIST_RANDOM, boards played 57 ticks "
         f"under POM_DIST_RANDOM; {a.reps} single calls per path after {a.warmup} warm-up calls, the paths alternating; us per call "
         f"(HIP events on the handle's stream)",
         f"{'shape':>14s} {'moves':5s} {'path':14s} {'median':>9s} {'min':>9s} {'max':>9s}"]
missed = []
for shape in a.shapes.split(","):
    n, R = (int(v) for v in shape.split("x"))
    roots = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=MAX_STEPS, stream=stream.cuda_stream)
    roots.make_game(pa.make_boards(n, seed=1))
    roots.step_random(3, DIST_RANDOM, 57, 1)
    outs = {k: torch.empty((R, n), dtype=torch.int32, device="cuda") for k in ("rollout", "rollout_again", "policy0")}
    for with_moves in (False, True):
        mv = torch.randint(0, 6, (n, 4), dtype=torch.int32, device="cuda", generator=torch.Generator("cuda").manual_seed(5)) if with_moves else None
        paths = {
            "rollout": lambda: roots.rollout(K, R, SEED, DIST_RANDOM, moves=mv, out=outs["rollout"]),
            "rollout_again": lambda: roots.rollout(K, R, SEED, DIST_RANDOM, moves=mv, out=outs["rollout_again"]),
            "policy0": lambda: roots.rollout(K, R, SEED, DIST_RANDOM, moves=mv, out=outs["policy0"], simple=0, first=0xF if with_moves else 0),
        }
        for _ in range(a.warmup):
            for call in paths.values():
                call()
        roots.sync()
        torch.cuda.synchronize()
        if not (torch.equal(outs["rollout"], outs["rollout_again"]) and torch.equal(outs["rollout"], outs["policy0"])):
            sys.exit(f"rollout_ab: {shape} moves {with_moves}: the three paths do not give the same words")
        t = {k: [] for k in paths}
        for rep in range(a.reps):
            for k, call in paths.items():
                t[k].append(timed(call, roots.sync))
        med = {k: statistics.median(v) for k, v in t.items()}
        tag = "yes" if with_moves else "no"
        for k in paths:
            lines.append(f"{n:>8d}x{R:<5d} {tag:5s} {k:14s} {med[k]:9.1f} {min(t[k]):9.1f} {max(t[k]):9.1f}")
        noise = abs(med["rollout_again"] / med["rollout"] - 1)
        excess = med["policy0"] / med["rollout"] - 1
        ok = excess <= 2 * noise
        if not ok:
            missed.append(f"{shape} moves {tag}")
        lines.append(f"{n:>8d}x{R:<5d} {tag:5s} noise (A/A) {100 * noise:.2f} %, policy0 / rollout - 1 = {100 * excess:+.2f} %: "
                     f"{'qualifies' if ok else 'DOES NOT QUALIFY'}")
    roots.close()
lines.append("policy0 qualifies at every row" if not missed else "policy0 DOES NOT QUALIFY at " + ", ".join(missed))
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
