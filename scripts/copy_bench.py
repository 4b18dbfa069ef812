"""Time pom_batch_copy_envs / _copy_envs_device (BatchEnvironment.copy_envs / restore) against the host path it replaces
(download, numpy gather, upload).

Cases, per batch size:
  fan_out        64 roots (envs 0..63) fanned out over envs 64..n-1: src[i] = i % 64
  permutation    an in-place resample with repeats over the whole batch: src = randint(0, n, n)
  restore_5pct   about 5 % of envs put back on their snapshot (from_snapshot, src[e] = e where masked, -1 elsewhere)
each through the host variant (numpy indices; fan-out takes the one-pass path, because no source is a destination) and the
device variant (a torch int64 tensor; always the two-pass path through the scratch).  Time per call = HIP events recorded on
the handle's stream around `reps` calls after `warmup` calls, divided by reps (host-side gaps between calls included).

Bytes per call are computed from the layout (include/pom_batch.h, pomcpp_amd/csrc/pom_copy.h), not measured:
  two-pass: every env of a touched tile 4 x 320 B (K1 loads the tile and stores the image, K2 loads the image and stores it),
            every copied env + 320 B (its source column or snapshot record) + 4 x 36 B (agent memory and episode, when copied)
  one-pass: every env of a touched tile 2 x 320 B, every copied env + 320 B + 2 x 36 B
`frac_8TBps` = those bytes / time / 8e12.  The host path moves 2 x 1004 B per env over PCIe plus the repacking on both sides.

    python scripts/copy_bench.py [--sizes 65536,1048576] [--reps 50] [--warmup 5] [--no-host] [--out FILE]
One JSON object per line on stdout (and in --out).

The two kernels' own times come from a kernel-trace run of this script, summarised afterwards (no GPU needed for that step):
    rocprofv3 --kernel-trace --stats -d DIR -o copy -- python scripts/copy_bench.py --reps 20 --no-host
    python scripts/copy_bench.py --trace-summary DIR/copy_results.db --reps 20
The summary assigns the copy kernels' dispatches to the cases by their order (the loop below: per size, per case, host then
device, warmup + reps calls each; the host fan-out is one kernel per call, every other call two).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

REC, AUX = 320, 36


def _bytes(n_touched_envs: int, copied: int, two_pass: bool, from_snapshot: bool) -> int:
    aux = 0 if from_snapshot else AUX  # from a snapshot: agent memory is only cleared, the episode stays
    if two_pass:
        return n_touched_envs * 4 * REC + copied * (REC + 4 * aux)
    return n_touched_envs * 2 * REC + copied * (REC + 2 * aux)


def _touched(first: int, count: int, n: int) -> int:
    t0, t1 = first // 16, (first + count - 1) // 16
    return min((t1 - t0 + 1) * 16, ((n + 15) // 16) * 16 - t0 * 16)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host path (download, gather, upload)")
    ap.add_argument("--out", default="")
    ap.add_argument("--trace-summary", default="", help="summarise a rocprofv3 kernel-trace database of a run with the same options")
    a = ap.parse_args()
    if a.trace_summary:
        return trace_summary(a)

    import torch
    import __graft_entry__ as g
    g.build_hip()
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, DIST_RANDOM

    dev = torch.device("cuda", 0)
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n in (int(s) for s in a.sizes.split(",")):
        rng = np.random.default_rng(1)
        with BatchEnvironment(n, mode=MODE_ENV, auto_reset=True, max_steps=800) as env:
            env.generate(3)
            env.step_random(5, DIST_RANDOM, ticks=20)
            env.step_simple(5, 2)  # agent memory allocated: the copy moves it
            env.sync()
            stream = torch.cuda.ExternalStream(env.stream_handle(), device=dev)

            def timed(call):
                for _ in range(a.warmup):
                    call()
                env.sync()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record(stream)
                for _ in range(a.reps):
                    call()
                e1.record(stream)
                e1.synchronize()
                wall = (time.perf_counter() - t0) / a.reps
                return e0.elapsed_time(e1) * 1e3 / a.reps, wall * 1e6

            fan = np.arange(n - 64, dtype=np.int64) % 64
            perm = rng.integers(0, n, n).astype(np.int64)
            mask = rng.random(n) < 0.05
            rest = np.where(mask, np.arange(n, dtype=np.int64), -1)
            cases = [
                ("fan_out", fan, 64, False, n - 64),
                ("permutation", perm, 0, False, n),
                ("restore_5pct", rest, 0, True, int(mask.sum())),
            ]
            for name, src, first, from_snap, copied in cases:
                src_dev = torch.from_numpy(src).to(dev)
                touched = _touched(first, src.size, n)
                for variant in ("host", "device"):
                    idx = src if variant == "host" else src_dev
                    us, wall_us = timed(lambda: env.copy_envs(idx, first, from_snapshot=from_snap))
                    one_pass = variant == "host" and name == "fan_out"
                    b = _bytes(touched, copied, not one_pass, from_snap)
                    emit(dict(case=name, n_envs=n, variant=variant, path="one-pass" if one_pass else "two-pass",
                              us_per_call=round(us, 2), host_wall_us_per_call=round(wall_us, 2), copied_envs=copied,
                              bytes_per_call=b, bytes_per_copied_env=round(b / max(copied, 1), 1),
                              GBps=round(b / us / 1e3, 1), frac_8TBps=round(b / (us * 1e-6) / 8e12, 4)))
            if not a.no_host:
                for name, src, first, _, copied in cases[:2]:
                    reps = 3 if n <= 65536 else 1
                    ts = []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        st = env.get_state()
                        env.make_game(np.ascontiguousarray(st[src]), first)
                        ts.append(time.perf_counter() - t0)
                    emit(dict(case=name, n_envs=n, variant="host_path (download, numpy gather, upload)",
                              us_per_call=round(min(ts) * 1e6, 1), copied_envs=copied, pcie_bytes_per_call=(n + src.size) * 1004))
    if a.out:
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")
    return 0


def trace_summary(a) -> int:
    import sqlite3
    db = sqlite3.connect(a.trace_summary)
    rows = db.execute("select name, duration, grid_x, vgpr_count, lds_size from kernels where name like '%pom_copy_%' "
                      "order by start").fetchall()
    calls = a.warmup + a.reps
    pos = 0
    for n in (int(s) for s in a.sizes.split(",")):
        for case in ("fan_out", "permutation", "restore_5pct"):
            for variant in ("host", "device"):
                per_call = 1 if (case, variant) == ("fan_out", "host") else 2
                seg = rows[pos:pos + calls * per_call][a.warmup * per_call:]
                pos += calls * per_call
                for k in sorted(set(r[0] for r in seg)):
                    d = [r[1] for r in seg if r[0] == k]
                    r0 = next(r for r in seg if r[0] == k)
                    short = "K1 gather" if "gather" in k else "K2 scatter" if "ILb1E" in k or "<true>" in k else "K2 snapshots only"
                    print(json.dumps(dict(case=case, n_envs=n, variant=variant, kernel=short, dispatches=len(d),
                                          mean_us=round(sum(d) / len(d) / 1e3, 2), min_us=round(min(d) / 1e3, 2),
                                          max_us=round(max(d) / 1e3, 2), workgroups=r0[2] // 64, vgprs=r0[3], lds_bytes=r0[4])))
    if pos != len(rows):
        print(json.dumps(dict(warning=f"{len(rows)} copy dispatches in the trace, {pos} expected: options differ from the traced run")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
