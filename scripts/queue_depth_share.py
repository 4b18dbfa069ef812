#!/usr/bin/env python3
"""How often does a wavefront-tick of the bench's workload hold an env with more than four flames or more than four bombs queued?

    python scripts/queue_depth_share.py [--envs 8192] [--ticks 100] [--burn-in 300] [--seed 1] [--kind ffa] [--dist 1]

The quad tick plays the first trip of its queue loops straight-line — lane `sub` of an env's quad takes queue offset `sub` — and enters
the loop behind it only for an env with more than four entries queued (pomcpp_amd/csrc/pom_step_body.h: flames_dec, step_middle's
scan and bomb pass).  A wavefront runs that loop if ANY of its 16 envs needs it.  Counted on the CPU with the oracle: bench.py's
boards (pomcpp_amd.make_boards, seed * 1000003) under its move stream (pom_oracle_run_random, the bench's seed and distribution,
restarts at 800 steps as in the bench), after the burn-in, 16 consecutive envs as a wavefront.  The flame count is taken where
flames_dec sees it (before the tick); the bomb count both before the tick and after it (the pass runs after the tick's plants and
before its explosions: the two bracket it).  No GPU needed."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--ticks", type=int, default=100)
    ap.add_argument("--burn-in", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--kind", default="ffa")
    ap.add_argument("--dist", type=int, default=1)
    args = ap.parse_args()
    import pomcpp_amd as pa
    from tests.oracle_lib import Oracle
    ora = Oracle()
    n = args.envs - args.envs % 16
    start = pa.make_boards(n, seed=args.seed * 1000003, kind=args.kind)
    cur = start.copy()
    ora.run_random(cur, start, args.burn_in, args.seed, 0, 0, args.dist, 800)
    waves = n // 16
    tot = dict(f=0, b_before=0, b_after=0, any_before=0, any_after=0, env_f=0, env_b=0, f_any=0, b_any=0)
    for t in range(args.ticks):
        f = cur["flames_count"].reshape(waves, 16)
        b0 = cur["bombs_count"].reshape(waves, 16).copy()
        wf = (f > 4).any(axis=1)
        tot["env_f"] += int((f > 4).sum())
        tot["f_any"] += int((f > 0).any(axis=1).sum())
        ora.run_random(cur, start, 1, args.seed, 0, args.burn_in + t, args.dist, 800)
        b1 = cur["bombs_count"].reshape(waves, 16)
        wb0, wb1 = (b0 > 4).any(axis=1), (np.maximum(b0, b1) > 4).any(axis=1)
        tot["env_b"] += int((b0 > 4).sum())
        tot["b_any"] += int((b0 > 0).any(axis=1).sum())
        tot["f"] += int(wf.sum())
        tot["b_before"] += int(wb0.sum())
        tot["b_after"] += int(wb1.sum())
        tot["any_before"] += int((wf | wb0).sum())
        tot["any_after"] += int((wf | wb1).sum())
    wt, et = waves * args.ticks, n * args.ticks
    pc = lambda v, d: f"{100.0 * v / d:6.2f} %"  # noqa: E731
    print(f"{n} envs ({waves} wavefronts of 16) x {args.ticks} ticks after {args.burn_in}, kind {args.kind}, dist {args.dist}, seed {args.seed}")
    print(f"wavefront-ticks with an env holding > 4 flames:                 {pc(tot['f'], wt)}   (env-ticks: {pc(tot['env_f'], et)})")
    print(f"wavefront-ticks with an env holding > 4 bombs, before the tick: {pc(tot['b_before'], wt)}   (env-ticks: {pc(tot['env_b'], et)})")
    print(f"                                   ... before or after it:      {pc(tot['b_after'], wt)}")
    print(f"wavefront-ticks with either:                                    {pc(tot['any_before'], wt)} .. {pc(tot['any_after'], wt)}")
    print(f"wavefront-ticks with any flame at all / any bomb at all:        {pc(tot['f_any'], wt)} / {pc(tot['b_any'], wt)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
