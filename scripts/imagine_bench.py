#!/usr/bin/env python3
"""Time pom_batch_imagine (BatchEnvironment.imagine) beside the only way to do the same without it: the view memory copied to the
host, the States built there — by the numpy checker of the call, tests/imagine_oracle.py, whose per-cell clauses work on whole arrays —
and pom_batch_upload (make_game) of those States.

The memory: --envs envs played --ticks ticks by step_simple, every agent remembering at radius 4 every tick.  Job j builds env j of a
second handle from view row j with sample j.  The call: single calls, as a search issues them — synchronise, one pair of HIP events
around the call, synchronise —, the median of --reps with their spread.  The host way: wall-clock time from the device memory to the
uploaded batch, synchronised, --host-reps times (it takes seconds).  Before anything is timed the call is checked against the checker
on the first --check-jobs jobs.
usage (on the GPU box): python scripts/imagine_bench.py [--envs N] [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
from tests import imagine_oracle as IO

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=40, help="SimpleAgent ticks played before the measurement")
ap.add_argument("--reps", type=int, default=16, help="single calls (the median is reported)")
ap.add_argument("--host-reps", type=int, default=1)
ap.add_argument("--jobs", type=int, nargs="*", default=[4096, 65536])
ap.add_argument("--check-jobs", type=int, default=2048, help="the jobs the numpy checker is compared with before the timing")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("imagine_bench: no GPU — nothing is measured without one")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
n, R, SEED = a.envs, 4, 1
dev = torch.device("cuda", 0)
env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
slots = BatchEnvironment(n, mode=MODE_ENV, stream=stream.cuda_stream)
slots.make_game(pa.make_boards(n, seed=2))
memory, stamp = pa.new_view_memory(n, dev)
attrs = torch.zeros((n, 4, 12), dtype=torch.int32, device=dev)
for _ in range(a.ticks):
    env.step_simple(SEED, 1)
    env.remember(memory, stamp, R, viewer_attrs=attrs)
env.sync()
torch.cuda.synchronize()


def host_way(jobs):
    """what a user does at the parent commit: memory and attributes to the host, States in numpy, upload"""
    rows = (jobs + 3) // 4
    m, va = memory[:rows].cpu().numpy(), attrs[:rows].cpu().numpy()
    states, words = IO.imagine(m, va, np.arange(jobs), None, SEED)
    built = (words & IO.BUILT) != 0
    if not built.all():   # (a refused job leaves its slot alone: upload the runs between them)
        states[~built] = slots.get_state(0, jobs)[~built]
    slots.make_game(states, 0)
    slots.sync()
    return states, words


# the check, before anything is timed
k = min(a.check_jobs, min(a.jobs))
view = torch.arange(max(a.jobs), dtype=torch.int32, device=dev)
out = slots.imagine(memory, attrs, view[:k], seed=SEED, stream=stream)
slots.sync()
got, got_words = slots.get_state(0, k), out.cpu().numpy().view(np.uint32)
want, want_words = IO.imagine(memory[:(k + 3) // 4].cpu().numpy(), attrs[:(k + 3) // 4].cpu().numpy(), np.arange(k), None, SEED)
built = (want_words & IO.BUILT) != 0
if not (np.array_equal(got_words, want_words) and got[built].tobytes() == want[built].tobytes()):
    sys.exit(f"imagine_bench: the call differs from the checker on the first {k} jobs")

lines = [f"imagine_bench: view memory of {n} envs after {a.ticks} SimpleAgent ticks, radius {R}; job j builds env j from view row j, sample j; unknown cells sampled",
         f"the call equals the numpy checker on the first {k} jobs ({int(built.sum())} built, mean {float(((want_words >> 8) & 0xFF)[built].mean()):.0f} unknown cells)",
         f"{'jobs':>7s} {'call us: median':>16s} {'min':>9s} {'max':>9s} {'host way ms':>12s} {'ratio':>9s} {'MB moved':>9s} {'TB/s':>6s} {'of 6.29':>8s}"]
PER_JOB = 726 + 48 + 4 + 4 + 3 * 320 + 32   # the view, its attributes, the list entry, the word; the record in, out and as snapshot; agent memory
for jobs in a.jobs:
    for _ in range(3):
        slots.imagine(memory, attrs, view[:jobs], seed=SEED, out=None, stream=stream)
    ts = []
    for rep in range(a.reps):
        slots.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        slots.imagine(memory, attrs, view[:jobs], seed=SEED + rep, stream=stream)
        e1.record(stream)
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    hs = []
    for rep in range(a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_way(jobs)
        hs.append((time.perf_counter() - t0) * 1e3)
    med, host = statistics.median(ts), statistics.median(hs)
    moved = jobs * PER_JOB
    lines.append(f"{jobs:7d} {med:16.1f} {min(ts):9.1f} {max(ts):9.1f} {host:12.1f} {host * 1e3 / med:9.0f} {moved / 1e6:9.1f} {moved / med / 1e6:6.2f} "
                 f"{100 * moved / med / 1e6 / 6.29:7.1f}%")
    print(lines[-1], flush=True)
lines.append(f"bytes per job: {PER_JOB} (the 726-byte view, 48 B of attributes, list entry and word, the 320-byte record read, written and written as "
             "snapshot, 32 B of agent memory); the ceiling is the 6.29 TB/s the project measured for a copy")
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
env.close()
slots.close()
