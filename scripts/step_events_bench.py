#!/usr/bin/env python3
"""What pom_batch_step_events costs over pom_batch_step_mixed, and what it replaces: "my network plays agent 0, SimpleAgent the other
three, every agent gets its fogged 9 x 9 view as codes — and the learner wants the tick's rewards" at 65,536 envs, POM_RESET_AT_END,
max_steps 800, boards 40 SimpleAgent ticks old.

Single whole-batch calls timed by device events on the handle's stream, the sequences ALTERNATING in one loop (the batch moves on one
tick with each, so all of them see the same mix of boards), median and spread of --reps:
  events        step_events(mask 0b1110, view_radius 4, ...) with events and outcome                       the new call, one launch
  events+wood   the same with the wood count
  mixed         step_mixed with the same arguments: the call without events
  mixed+last    step_mixed + last_results(): what had to be done before to learn how a game ended (a copy to the host and a wait)
--parent-lib PATH also runs `mixed` alone, in a process of its own, on a library built from the parent commit (the kernels of
step_mixed in this build are the parent's instruction for instruction — scripts/compare_kernel_isa.py — so this only shows the run-to-run
spread between two processes).  The text goes to the terminal and to --out.  usage (GPU box): python scripts/step_events_bench.py"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import pomcpp_amd as pa  # noqa: E402
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--reps", type=int, default=16)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_events_bench.txt"))
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--only-mixed", action="store_true", help="(the child process of --parent-lib)")
a = ap.parse_args()
n, MASK, SEED, RADIUS = a.envs, 0b1110, 7, 4
dev = torch.device("cuda", 0)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


env = BatchEnvironment(n, device=0, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800)
env.make_game(pa.make_boards(n, seed=1000003))
env.step_simple(SEED, 40)
env.sync()
views = torch.zeros((n, 4, 5, 11, 11), dtype=torch.uint8, device=dev)
v_attrs = torch.zeros((n, 4, 12), dtype=torch.int32, device=dev)
e_attrs = torch.zeros((n, 4), dtype=torch.int32, device=dev)
moves = torch.randint(0, 6, (n, 4), dtype=torch.int32, device=dev)
events = torch.zeros((n, 4), dtype=torch.int32, device=dev)
outcome = torch.zeros((n,), dtype=torch.int32, device=dev)
wood = torch.zeros((n,), dtype=torch.uint8, device=dev)
torch.cuda.synchronize()
hs = torch.cuda.ExternalStream(env.stream_handle(), device=dev)
tick = [100]
obs = dict(codes=views, view_radius=RADIUS, viewer_attrs=v_attrs, env_attrs=e_attrs)


def mixed():
    env.step_mixed(0, n, moves, MASK, SEED, tick[0], None, **obs)


def mixed_last():
    env.step_mixed(0, n, moves, MASK, SEED, tick[0], None, **obs)
    env.last_results()


def with_events():
    env.step_events(0, n, moves, MASK, SEED, tick[0], events, outcome, None, None, **obs)


def with_wood():
    env.step_events(0, n, moves, MASK, SEED, tick[0], events, outcome, wood, None, **obs)


SEQUENCES = (("mixed", mixed),) if a.only_mixed else (("events", with_events), ("events+wood", with_wood), ("mixed", mixed), ("mixed+last", mixed_last))
times = {name: [] for name, _ in SEQUENCES}
with torch.cuda.stream(hs):
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
med = {k: statistics.median(v) for k, v in times.items()}
if a.only_mixed:
    t = sorted(times["mixed"])
    print(f"  mixed         median {med['mixed']:8.2f} us   min {t[0]:8.2f}   max {t[-1]:8.2f}", flush=True)
    sys.exit(0)
say(f"{n} envs, POM_RESET_AT_END, max_steps 800, boards 40 SimpleAgent ticks old, mask {MASK:#06b}, fogged code views radius {RADIUS} "
    f"with viewer_attrs and env_attrs; single whole-batch calls, device events, {a.reps} alternating repetitions")
for name, _ in SEQUENCES:
    t = sorted(times[name])
    say(f"  {name:12s} median {med[name]:8.2f} us   min {t[0]:8.2f}   max {t[-1]:8.2f}")
say(f"  events / mixed = {med['events'] / med['mixed']:.3f}   events+wood / mixed = {med['events+wood'] / med['mixed']:.3f}   "
    f"events / (mixed + last_results) = {med['events'] / med['mixed+last']:.3f}")
for name in ("events", "events+wood"):
    over = (med[name] / med["mixed"] - 1) * 100
    say(f"  {name} costs {over:+.1f} % over step_mixed in the same run: " + ("within" if over <= 5 else "ABOVE") + " the 5 % margin")
ended = int((events.cpu() & pa.EV_END != 0).any(1).sum())
say(f"  (the last tick's record: {ended} envs ended, {int(wood.sum())} wood cells burnt)")
env.close()
if a.parent_lib:
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--envs", str(n), "--reps", str(a.reps), "--only-mixed"],
                           env=dict(os.environ, POM_LIB=os.path.abspath(a.parent_lib)), capture_output=True, text=True)
    say("step_mixed of a library built from the parent commit, in a process of its own:")
    say(child.stdout.rstrip() if child.returncode == 0 else f"  failed ({child.returncode}): {child.stderr[-400:]}")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
