#!/usr/bin/env python3
"""Time pom_batch_reach (dist alone, move alone, both; agent masks 0x1 and 0xF; max_dist 10 and 120) on played boards, beside one
pom_batch_policy_simple launch on the same boards — the existing kernel that runs floods for four agents — and beside the old way on a
slice of the batch: download the States and run the oracle's FillRMap (pom_oracle_fill_rmap) on 16 host threads, one ctypes call per
(env, agent).

Single calls, as a search or a learner issues them: synchronise, one pair of HIP events around the call, synchronise; the paths
alternate inside every repetition and the median of the repetitions is reported with their spread.  The figures hold the start of a
call from an idle device.  The host path is timed with the wall clock, download included.
usage (on the GPU box): python scripts/reach_bench.py [--envs N] [--reps R] [--out FILE]"""
import argparse
import concurrent.futures
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import MODE_ENV, BatchEnvironment
from tests.oracle_lib import Oracle

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=40, help="SimpleAgent ticks played before the measurement")
ap.add_argument("--reps", type=int, default=16, help="single calls per path (the median is reported)")
ap.add_argument("--host-envs", type=int, default=4096, help="the slice the host path works on")
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("reach_bench: no GPU — nothing is measured without one")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
n = a.envs
env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
env.step_simple(1, a.ticks)
out = env.reach()

paths = {}
for max_dist in (10, 120):
    for mask in (0x1, 0xF):
        for what, kw in (("dist", dict(move=False)), ("move", dict(dist=False)), ("dist+move", {})):
            o = {k: v for k, v in out.items() if k in what}
            paths[f"reach max_dist {max_dist:3d} mask {mask:#x} {what}"] = lambda max_dist=max_dist, mask=mask, kw=kw, o=o: env.reach(mask, max_dist, o, **kw)
paths["policy_simple, one launch"] = lambda: env.policy_simple(1)
for call in paths.values():  # warm-up: every kernel the timed window uses
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

# the old way: the States over PCIe, then a breadth-first search per agent on host cores
lib = Oracle().lib
lib.pom_oracle_fill_rmap.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.pom_oracle_fill_rmap.restype = None
hn = min(a.host_envs, n)
maps, moves = np.zeros((hn, 4, 121), dtype=np.int32), np.zeros((hn, 4, 121), dtype=np.int32)


def host_chunk(states, lo, hi):
    base = states.ctypes.data
    for e in range(lo, hi):
        for ag in range(4):
            lib.pom_oracle_fill_rmap(base + 1004 * e, ag, maps[e, ag].ctypes.data, moves[e, ag].ctypes.data)


host = []
with concurrent.futures.ThreadPoolExecutor(a.threads) as pool:
    for rep in range(3):
        env.sync()
        t0 = time.perf_counter()
        states = env.get_state(0, hn)
        t1 = time.perf_counter()
        cuts = np.linspace(0, hn, a.threads + 1).astype(int)
        list(pool.map(lambda k: host_chunk(states, cuts[k], cuts[k + 1]), range(a.threads)))
        host.append(((t1 - t0) * 1e6, (time.perf_counter() - t1) * 1e6))

env.reach(out=out)  # what the boards are like
d = out["dist"]
alive = torch.from_numpy(env.get_state()["agents"]["dead"] == 0).to(d.device)
reached = (d != 0).flatten(2).sum(2)[alive].float()
far = d.flatten(2).amax(2)[alive].float()
lines = [f"reach_bench: {n} envs, ffa boards after {a.ticks} SimpleAgent ticks, {a.reps} single calls per path, us per call",
         f"{int(alive.sum())} live agents; cells reached per live agent: mean {reached.mean():.1f}, max {int(reached.max())}; farthest cell: "
         f"mean {far.mean():.1f}, max {int(far.max())} (a wavefront of 16 floods runs as many levels as its longest)",
         f"{'path':48s} {'median':>9s} {'min':>9s} {'max':>9s}"]
med = {}
for name, ts in times.items():
    med[name] = statistics.median(ts)
    lines.append(f"{name:48s} {med[name]:9.1f} {min(ts):9.1f} {max(ts):9.1f}")
for max_dist in (10, 120):
    for mask in (0x1, 0xF):
        dd, mm, bb = (med[f"reach max_dist {max_dist:3d} mask {mask:#x} {w}"] for w in ("dist", "move", "dist+move"))
        lines.append(f"max_dist {max_dist} mask {mask:#x}: move / dist = {mm:.1f} / {dd:.1f} = {mm / dd:.2f}; both / dist = {bb / dd:.2f}; "
                     f"both / policy_simple = {bb / med['policy_simple, one launch']:.2f}")
dl, bfs = min(h[0] for h in host), min(h[1] for h in host)
lines.append(f"the old way, {hn} envs, best of 3: download {dl:.0f} us + pom_oracle_fill_rmap x 4 agents on {a.threads} host threads (ctypes, a call per "
             f"(env, agent)) {bfs:.0f} us = {(dl + bfs) / hn:.2f} us per env; reach dist+move mask 0xf: {med['reach max_dist 120 mask 0xf dist+move'] / n:.4f} us per env")
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
env.close()
