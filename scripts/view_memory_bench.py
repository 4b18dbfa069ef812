#!/usr/bin/env python3
"""Time pom_batch_remember_view (BatchEnvironment.remember) beside what it replaces: the fogged view export (observe_view, code planes,
with viewer_attrs) followed by the same merge written in torch — the recipe a user of the closed loop writes today —, beside the bare
view export on the same boards, and as a loop tick: step_mixed + remember against step_mixed with fused views + the torch merge.

The boards: SimpleAgent x4 for --ticks ticks, envs restarting at the end of the tick that finishes them, the memory updated every tick
on the way, so that it holds what a running loop's holds.  Single calls, as a loop issues them: synchronise, one pair of HIP events
around the sequence, synchronise; the sequences alternate inside every repetition and the median of the repetitions is reported with
their spread.  Before every timed single merge the memory and the stamps are put back to the tick before (outside the events), so
that every call is a real merge with dt = 1.  The torch merge is checked against the numpy checker (tests/view_memory_oracle.py) on
the first --check-envs envs before anything is timed, and so is the call.
usage (on the GPU box): python scripts/view_memory_bench.py [--envs N] [--reps R] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import pomcpp_amd as pa
from pomcpp_amd.batch import MODE_ENV, RESET_AT_END, BatchEnvironment
from tests import view_memory_oracle as VM

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--ticks", type=int, default=40, help="SimpleAgent ticks played before the measurement")
ap.add_argument("--reps", type=int, default=16, help="single calls per sequence (the median is reported)")
ap.add_argument("--radius", type=int, default=4)
ap.add_argument("--check-envs", type=int, default=4096, help="the slice the numpy checker works on")
ap.add_argument("--out", default=None)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("view_memory_bench: no GPU — nothing is measured without one")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
n, R, SEED = a.envs, a.radius, 1
env = BatchEnvironment(n, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800, stream=stream.cuda_stream)
env.make_game(pa.make_boards(n, seed=1))
dev = torch.device("cuda", 0)
XS = torch.arange(11, device=dev, dtype=torch.int32)
WIPED = torch.tensor([5, 0, 0, 0, 0, 255], device=dev, dtype=torch.int16).view(1, 1, 6, 1)


def torch_merge(memory, stamp, views, viewer_attrs, ep):
    """THE RULE of include/pom_batch.h in torch, from what the view export gives: the fogged code planes uint8 [n, 4, 5, 11, 11] and
    viewer_attrs int32 [n, 4, 12] (x, y, alive first, timeStep last), and the episode counters int32 [n]"""
    x, y, alive, t = viewer_attrs[:, :, 0], viewer_attrs[:, :, 1], viewer_attrs[:, :, 2] != 0, viewer_attrs[:, :, 11]
    inside = (((XS.view(1, 1, 1, 11) - x[:, :, None, None]).abs() <= R) & ((XS.view(1, 1, 11, 1) - y[:, :, None, None]).abs() <= R)).flatten(2)
    # who is gone for viewer v: agent a dead, or standing inside v's window
    seen = ((x[:, None, :] - x[:, :, None]).abs() <= R) & ((y[:, None, :] - y[:, :, None]).abs() <= R)
    gone = seen | ~alive[:, None, :]                                                   # [n, v, a]
    wipe = (stamp[:, :, 0] != ep[:, None]) | (t < stamp[:, :, 1])
    dt = torch.where(wipe, 0, (t - stamp[:, :, 1]).clamp(max=255)).to(torch.int16)[:, :, None]
    old = memory.flatten(3).to(torch.int16)                                            # [n, 4, 6, 121]
    b, s, life, d, f, age = old.unbind(2)
    aging = ~inside & ~wipe[:, :, None] & (age != 255) & (dt > 0)
    life2 = (life - dt).clamp(min=0)
    out = (life > 0) & (life2 == 0)
    s2, d2 = torch.where(out, 0, s), torch.where(out, 0, d)
    b2 = torch.where(out & (b == 3), 0, b)
    fl = b2 == 4
    f2 = torch.where(fl, (f - dt).clamp(min=0), f)
    b2 = torch.where(fl & (f2 == 0), 0, b2)
    ag = b2 - 10
    stale = (ag >= 0) & (ag < 4) & gone.gather(2, ag.clamp(0, 3).long())
    b2 = torch.where(stale, torch.where(life2 > 0, 3, 0).to(torch.int16), b2)
    age2 = (age + dt).clamp(max=254)
    res = torch.where(aging[:, :, None], torch.stack([b2, s2, life2, d2, f2, age2], dim=2), old)
    res = torch.where(wipe[:, :, None, None], WIPED, res)
    now = torch.cat([views.flatten(3).to(torch.int16), torch.zeros_like(b)[:, :, None]], dim=2)
    res = torch.where(inside[:, :, None], now, res)
    memory.copy_(res.to(torch.uint8).view_as(memory))
    stamp[:, :, 0] = ep[:, None]
    stamp[:, :, 1] = t


# the boards, and a memory that has followed them
memory, stamp = pa.new_view_memory(n, dev)
for _ in range(a.ticks - 1):
    env.remember(memory, stamp, R)
    env.step_simple(SEED, 1)
env.remember(memory, stamp, R)
env.step_simple(SEED, 1)   # the memory is one tick behind: a call now is a merge with dt = 1
memory0, stamp0 = memory.clone(), stamp.clone()
ep = torch.from_numpy(env.episodes().astype(np.int32)).to(dev)
views, viewer_attrs, _ = env.observe(dtype="codes", view_radius=R)
va = torch.empty_like(viewer_attrs)
mem_t, stamp_t = memory.clone(), stamp.clone()


def back():
    for dst, src in ((memory, memory0), (stamp, stamp0), (mem_t, memory0), (stamp_t, stamp0)):
        dst.copy_(src)


def seq_call():
    env.remember(memory, stamp, R, viewer_attrs=va)


def seq_torch():
    _, attrs, _ = env.observe(dtype="codes", view_radius=R, out=views)   # (allocates its attribute tensors anew: part of what a loop pays)
    torch_merge(mem_t, stamp_t, views, attrs, ep)


def seq_view():
    env.observe(dtype="codes", view_radius=R, out=views)


# the loop tick: all four agents SimpleAgent, one range.  Every timed tick moves the games on, so the two sequences, alternating, see
# every other tick each: each has a memory of its own, and its merges are real ones with dt = 2
mem_a, stamp_a, mem_b, stamp_b = memory0.clone(), stamp0.clone(), memory0.clone(), stamp0.clone()
tick = [a.ticks]


def loop_call():
    env.step_mixed(0, n, None, 15, SEED, tick[0], stream)
    env.remember(mem_a, stamp_a, R, stream=stream, viewer_attrs=va)
    tick[0] += 1


def loop_torch():
    env.step_mixed(0, n, None, 15, SEED, tick[0], stream, codes=views, view_radius=R, viewer_attrs=viewer_attrs)
    torch_merge(mem_b, stamp_b, views, viewer_attrs, ep)
    tick[0] += 1


single = {"remember (the call, with viewer_attrs)": seq_call, "observe_view codes + torch merge": seq_torch, "observe_view codes alone": seq_view}
loops = {"tick: step_mixed + remember": loop_call, "tick: step_mixed with fused views + torch merge": loop_torch}

# the check, before anything is timed: the call and the torch merge against the numpy checker on a slice
k = min(a.check_envs, n)
codes, agent_attrs, env_attrs = env.observe(dtype="codes")
want_m, want_s = memory0[:k].cpu().numpy(), stamp0[:k].cpu().numpy()
VM.remember(want_m, want_s, codes[:k].cpu().numpy(), agent_attrs[:k].cpu().numpy(), env_attrs[:k].cpu().numpy(), env.episodes(0, k), R)
back()
seq_call()
seq_torch()
env.sync()
torch.cuda.synchronize()
for what, m, s in (("the call", memory, stamp), ("the torch merge", mem_t, stamp_t)):
    if not (np.array_equal(m[:k].cpu().numpy(), want_m) and np.array_equal(s[:k].cpu().numpy(), want_s)):
        sys.exit(f"view_memory_bench: {what} differs from the checker on the first {k} envs")
if not (torch.equal(memory, mem_t) and torch.equal(stamp, stamp_t) and torch.equal(va, viewer_attrs)):
    sys.exit("view_memory_bench: the call and the torch merge differ")
changed = int((memory != memory0).any(dim=2).sum())

for call in list(single.values()) + list(loops.values()):  # warm-up: every kernel the timed window uses
    for _ in range(3):
        call()
times = {name: [] for name in list(single) + list(loops)}
for rep in range(a.reps):  # the sequences alternate inside a repetition: what disturbs one disturbs its neighbours too
    for name, call in list(single.items()) + list(loops.items()):
        if name in single:
            back()
        env.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        torch.cuda.synchronize()
        times[name].append(e0.elapsed_time(e1) * 1e3)

lines = [f"view_memory_bench: {n} envs, ffa boards after {a.ticks} SimpleAgent ticks (reset at the end of the tick), radius {R}, all four agents, "
         f"{a.reps} single calls per sequence, us per call",
         f"the call and the torch merge equal the numpy checker on the first {k} envs and each other on all; a merge changes {changed} of {n * 4 * 121} cells",
         f"{'sequence':52s} {'median':>9s} {'min':>9s} {'max':>9s}"]
med = {}
for name, ts in times.items():
    med[name] = statistics.median(ts)
    lines.append(f"{name:52s} {med[name]:9.1f} {min(ts):9.1f} {max(ts):9.1f}")
c, tm, v = (med[k_] for k_ in single)
lc, lt = (med[k_] for k_ in loops)
moved = n * (2 * 2904 + 320 + 4 * 48 + 2 * 32 + 4)   # memory in and out, the record, viewer_attrs out, stamps in and out, the episode counter
lines.append(f"the call / (observe_view + torch merge) = {c:.1f} / {tm:.1f} = {c / tm:.3f}; the call / observe_view alone = {c / v:.2f}")
lines.append(f"loop tick: (step_mixed + remember) / (step_mixed with views + torch merge) = {lc:.1f} / {lt:.1f} = {lc / lt:.3f}")
lines.append(f"the call moves {moved / 1e6:.0f} MB: {moved / c / 1e6:.2f} TB/s, {100 * moved / c / 1e6 / 8:.0f} % of the 8 TB/s line")
text = "\n".join(lines)
print(text, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
env.close()
