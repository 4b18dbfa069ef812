#!/usr/bin/env python3
"""The compact views (pom_batch.h PomCompactViewSpec) against the four fogged views they select from, in scripts/mixed_bench.py's
setup: 65,536 envs, POM_RESET_AT_END, max_steps 800, boards 40 SimpleAgent ticks old, mask 0b1110, radius 4, viewer_attrs and
env_attrs.  Whole-batch calls timed by device events on the handle's stream, the sequences ALTERNATING in one loop (the batch moves on
with each step_mixed, so every form sees the same mix of boards), median and spread of --reps.  For step_mixed and for observe():
  four       the four fogged views, uint8 [n,4,5,11,11]: the form before this one, the baseline of the same run
  one        viewers=[0], uncentred, [n,1,5,11,11]
  one-c      viewers=[0], centred, [n,1,5,9,9]
  four-c     all four viewers, centred, [n,4,5,9,9]
  none       no views at all (step_mixed only: the tick, the policy and the record's round trip)
Per row: the bytes the call writes as observation (planes + viewer_attrs + env_attrs), the time, and those bytes over that time as
a share of the 6.29 TB/s a device copy reaches.  usage (GPU box): python scripts/compact_view_bench.py [--envs N] [--reps R]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import pomcpp_amd as pa  # noqa: E402
from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--reps", type=int, default=16)
a = ap.parse_args()
n, MASK, SEED, RADIUS, COPY_TBS = a.envs, 0b1110, 7, 4, 6.29
dev = torch.device("cuda", 0)

env = BatchEnvironment(n, device=0, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=800)
env.make_game(pa.make_boards(n, seed=1000003))
env.step_simple(SEED, 40)
env.sync()
hs = torch.cuda.ExternalStream(env.stream_handle(), device=dev)
moves = torch.randint(0, 6, (n, 4), dtype=torch.int32, device=dev)
e_attrs = torch.zeros((n, 4), dtype=torch.int32, device=dev)

FORMS = {}   # name -> (the observation's keyword arguments, bytes written)
for name, k, s, extra in (("four", 4, 11, {}), ("one", 1, 11, dict(viewers=[0])), ("one-c", 1, 9, dict(viewers=[0], centred=True)),
                          ("four-c", 4, 9, dict(viewers=15, centred=True))):
    planes = torch.zeros((n, k, 5, s, s), dtype=torch.uint8, device=dev)
    v_attrs = torch.zeros((n, k, 12), dtype=torch.int32, device=dev)
    FORMS[name] = (dict(codes=planes, view_radius=RADIUS, viewer_attrs=v_attrs, env_attrs=e_attrs, **extra),
                   planes.numel() + 4 * v_attrs.numel() + 4 * e_attrs.numel())
torch.cuda.synchronize()
tick = [100]


def mixed(kw):
    env.step_mixed(0, n, moves, MASK, SEED, tick[0], None, **kw)
    tick[0] += 1


def observe(kw):
    # the stand-alone call through the spec, so that no allocation of the wrapper's is timed
    compact = None if "viewers" not in kw else (15 if kw["viewers"] == 15 else 1, int(bool(kw.get("centred"))))
    spec = pa._abi._view_spec(3, RADIUS, kw["codes"], kw["viewer_attrs"], kw["env_attrs"], compact)
    pa._abi._check(env._lib, env._lib.pom_batch_observe_view(env._h, C.byref(spec)))


SEQUENCES = [("step_mixed " + f, mixed, FORMS[f][0], FORMS[f][1]) for f in FORMS] + [("step_mixed none", mixed, {}, 0)]
SEQUENCES += [("observe    " + f, observe, FORMS[f][0], FORMS[f][1]) for f in FORMS]
times = {name: [] for name, *_ in SEQUENCES}
with torch.cuda.stream(hs):
    for rep in range(-3, a.reps):   # three warm-up rounds
        for name, fn, kw, _ in SEQUENCES:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            env.sync()
            ev0.record(hs)
            fn(kw)
            env.flush()
            ev1.record(hs)
            torch.cuda.synchronize()
            if rep >= 0:
                times[name].append(ev0.elapsed_time(ev1) * 1e3)
print(f"{n} envs, POM_RESET_AT_END, max_steps 800, boards 40 SimpleAgent ticks old, mask {MASK:#06b}, code views radius {RADIUS} with "
      f"viewer_attrs and env_attrs; single whole-batch calls, device events, {a.reps} alternating repetitions", flush=True)
med = {}
for name, _, _, nbytes in SEQUENCES:
    t = sorted(times[name])
    med[name] = statistics.median(t)
    share = nbytes / (med[name] * 1e-6) / (COPY_TBS * 1e12)
    print(f"  {name:18s} {nbytes / 1e6:8.2f} MB   median {med[name]:8.2f} us   min {t[0]:8.2f}   max {t[-1]:8.2f}   {100 * share:5.1f} % of {COPY_TBS} TB/s", flush=True)
for call in ("step_mixed", "observe   "):
    four = sorted(times[f"{call} four"])
    for f in ("one", "one-c"):
        t = sorted(times[f"{call} {f}"])
        clear = t[-1] < four[0]   # every repetition of the one below every repetition of the other: beyond the spread
        print(f"  {call.strip()} {f}: {med[f'{call} {f}'] - med[f'{call} four']:+.2f} us against four views, "
              + ("BEYOND" if clear else "WITHIN") + " the spread of the repetitions", flush=True)
span = med["step_mixed four"] - med["step_mixed none"]
for f in ("one", "one-c", "four-c"):
    print(f"  step_mixed {f} lies {(med['step_mixed ' + f] - med['step_mixed none']) / span:.2f} of the way from no views to four views", flush=True)
env.close()
