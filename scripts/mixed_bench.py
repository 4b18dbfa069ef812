#!/usr/bin/env python3
"""pom_batch_step_mixed against the ways the same RL tick is played without it: "my network plays agent 0, SimpleAgent the other three,
every agent gets its fogged 9 x 9 view as codes" at 65,536 envs, POM_RESET_AT_END, max_steps 800, boards 40 SimpleAgent ticks old.

Single calls, whole batch, timed by device events on the handle's stream, the four sequences ALTERNATING in one loop (the batch moves on
one tick with each, so all of them see the same mix of boards), median and spread of --reps:
  mixed      step_mixed(mask 0b1110, view_radius 4, viewer_attrs, env_attrs)                                  the new call, one launch
  today      policy_simple + overwrite of agent 0's column of the move buffer + step_policy + observe(view_radius 4)
  floor      step_device_range(view_radius 4) with all four moves explicit: no SimpleAgent at all
  simple     step_simple(1) + observe(view_radius 4): what the policy itself costs, all four agents asked
Then the closed loop, per tick over --ticks x --loop-reps ticks: two ranges on two streams, pom_bench_policy standing in for the learner
in front of every step (it writes the range's moves from (env, agent, tick); the fogged views are not its input format), with the mixed
call issued by one thread and as a replayed graph, the range call as the floor, and today's whole-batch sequence behind a whole-batch
pom_bench_policy.  usage (GPU box): python scripts/mixed_bench.py [--envs N]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import pomcpp_amd as pa  # noqa: E402
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END, bench_policy  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--reps", type=int, default=16)
ap.add_argument("--ticks", type=int, default=25)
ap.add_argument("--loop-reps", type=int, default=8)
a = ap.parse_args()
n, MASK, SEED, RADIUS = a.envs, 0b1110, 7, 4
dev = torch.device("cuda", 0)


def handle():
    env = BatchEnvironment(n, device=0, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800)
    env.make_game(pa.make_boards(n, seed=1000003))
    env.step_simple(SEED, 40)
    env.sync()
    return env


views = torch.zeros((n, 4, 5, 11, 11), dtype=torch.uint8, device=dev)
v_attrs = torch.zeros((n, 4, 12), dtype=torch.int32, device=dev)
e_attrs = torch.zeros((n, 4), dtype=torch.int32, device=dev)
moves = torch.randint(0, 6, (n, 4), dtype=torch.int32, device=dev)
torch.cuda.synchronize()

# ---- single calls -----------------------------------------------------------------------------------------------------------------
env = handle()
hs = torch.cuda.ExternalStream(env.stream_handle(), device=dev)
buf = env.moves_tensor()
tick = [100]


def mixed():
    env.step_mixed(0, n, moves, MASK, SEED, tick[0], None, codes=views, view_radius=RADIUS, viewer_attrs=v_attrs, env_attrs=e_attrs)


def today():
    env.set_tick(tick[0])
    env.policy_simple(SEED)
    env.flush()            # the policy ran on the handle's sub-streams: the overwrite on its stream comes behind it
    buf[:, 0] = moves[:, 0]
    env.step_policy()
    env.observe(dtype="codes", out=views, view_radius=RADIUS)


def floor():
    env.step_device_range(0, n, moves, None, codes=views, view_radius=RADIUS, viewer_attrs=v_attrs, env_attrs=e_attrs)


def simple():
    env.set_tick(tick[0])
    env.step_simple(SEED, 1)
    env.observe(dtype="codes", out=views, view_radius=RADIUS)


SEQUENCES = (("mixed", mixed), ("today", today), ("floor", floor), ("simple", simple))
times = {name: [] for name, _ in SEQUENCES}
with torch.cuda.stream(hs):   # torch's work (the overwrite, observe()'s attribute tensors) goes to the handle's own stream
    for rep in range(-3, a.reps):   # three warm-up rounds
        for name, fn in SEQUENCES:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            env.sync()
            ev0.record(hs)
            fn()
            env.flush()
            ev1.record(hs)
            torch.cuda.synchronize()
            tick[0] += 1
            if rep >= 0:
                times[name].append(ev0.elapsed_time(ev1) * 1e3)
print(f"{n} envs, POM_RESET_AT_END, max_steps 800, boards 40 SimpleAgent ticks old, mask {MASK:#06b}, fogged code views radius {RADIUS} "
      f"with viewer_attrs and env_attrs; single whole-batch calls, device events, {a.reps} alternating repetitions", flush=True)
for name, _ in SEQUENCES:
    t = sorted(times[name])
    print(f"  {name:7s} median {statistics.median(t):8.2f} us   min {t[0]:8.2f}   max {t[-1]:8.2f}", flush=True)
med = {k: statistics.median(v) for k, v in times.items()}
print(f"  mixed / today = {med['mixed'] / med['today']:.3f}   mixed - floor = {med['mixed'] - med['floor']:.2f} us   "
      f"simple - floor = {med['simple'] - med['floor']:.2f} us", flush=True)
print("  the new call's median lies " + ("BELOW" if med["mixed"] < med["today"] else "NOT below") + " today's sequence's", flush=True)
del buf
env.close()

# ---- the closed loop: two ranges on two streams, a stand-in learner in front of every step --------------------------------------------
half = n // 2 // 16 * 16
ranges = [(0, half), (half, n - half)]


def loop(how):
    env = handle()
    lmoves = torch.zeros((n, 4), dtype=torch.int32, device=dev)
    side, main = [torch.cuda.Stream(device=dev) for _ in ranges], torch.cuda.Stream(device=dev)
    hs = torch.cuda.ExternalStream(env.stream_handle(), device=dev)
    buf = env.moves_tensor() if how == "today" else None
    torch.cuda.synchronize()

    def issue(ticks, t0=0):
        if how == "today":   # no range form: whole-batch calls on the handle's stream
            with torch.cuda.stream(hs):
                for t in range(t0, t0 + ticks):
                    bench_policy(None, lmoves, 0, n, t, hs)
                    env.set_tick(t)
                    env.policy_simple(SEED)
                    env.flush()
                    buf[:, 0] = lmoves[:, 0]
                    env.step_policy()
                    env.observe(dtype="codes", out=views, view_radius=RADIUS)
                env.flush()
            return
        for s in side:
            s.wait_stream(main)
        for t in range(t0, t0 + ticks):
            for (f, c), s in zip(ranges, side):
                bench_policy(None, lmoves, f, c, t, s)
                if how == "floor":
                    env.step_device_range(f, c, lmoves, s, codes=views, view_radius=RADIUS, viewer_attrs=v_attrs, env_attrs=e_attrs)
                else:
                    env.step_mixed(f, c, lmoves, MASK, SEED, t, s, codes=views, view_radius=RADIUS, viewer_attrs=v_attrs, env_attrs=e_attrs)
        for s in side:
            main.wait_stream(s)

    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    where = hs if how == "today" else main
    if how == "mixed, graph":
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=main):
            issue(a.ticks)
        g.replay()
        torch.cuda.synchronize()
        with torch.cuda.stream(main):
            ev0.record(main)
            for _ in range(a.loop_reps):
                g.replay()
            ev1.record(main)
    else:
        issue(a.ticks)
        torch.cuda.synchronize()
        with torch.cuda.stream(where):
            ev0.record(where)
            issue(a.ticks * a.loop_reps, a.ticks)
            ev1.record(where)
    torch.cuda.synchronize()
    us = ev0.elapsed_time(ev1) * 1e3 / (a.ticks * a.loop_reps)
    print(f"  {how:18s} {us:8.2f} us per tick = {n / us / 1e3:.3f} G env-steps/s", flush=True)
    del buf
    env.close()


print(f"closed loop, {a.ticks * a.loop_reps} ticks: two ranges on two streams, pom_bench_policy in front of every step", flush=True)
for how in ("mixed, one thread", "mixed, graph", "floor", "today"):
    loop(how)
