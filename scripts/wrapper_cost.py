#!/usr/bin/env python
"""Host cost of the wrapper's closed-loop calls, this tree's pomcpp_amd/batch.py against a parent's, on the CPU alone: the library is
a stand-in whose every function does nothing, the tensors are ducks (tests/wrapper_standin.py), so what is timed is the Python between
the caller and the library — argument checks, the spec, the ctypes call's set-up.  step_device and four forms of step_device_range
(moves only; with `codes`; fogged views with both attribute arrays; raw addresses), RUNS runs of CALLS calls each, parent and branch
alternating.  The rule is profiles/host_split_ab.txt's with the margin taken from the parent: the branch's median is at most the
parent's median plus the parent's own spread (max - min of its runs).  On a host whose clock wanders the minimum of the runs, printed
beside it, is the steadier figure.

    python scripts/wrapper_cost.py [--parent REV_OR_DIR] [--runs 5] [--calls 20000]

--parent: a git revision (default HEAD^; its pomcpp_amd/*.py are written to a scratch package) or a directory holding such a package."""
import argparse
import gc
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("POM_NO_TORCH", "1")

from tests import wrapper_standin as W  # noqa: E402

N = 65536


class Nothing:
    """the library: every function exists, does nothing and returns POM_OK"""

    def __getattr__(self, name):
        fn = lambda *a: 0  # noqa: E731
        setattr(self, name, fn)
        return fn


def parent_package(parent: str, scratch: str):
    """(the directory of the parent's package, what to call the parent in the table: the commit, or the directory's name)"""
    if os.path.isdir(parent):
        return parent, os.path.basename(os.path.normpath(parent))
    commit = subprocess.run(["git", "rev-parse", "--short", parent], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    directory = os.path.join(scratch, "pom_parent")
    os.makedirs(directory)
    names = subprocess.run(["git", "ls-tree", "--name-only", parent, "pomcpp_amd/"], cwd=ROOT, check=True, capture_output=True, text=True).stdout.split()
    for name in names:
        if name.endswith(".py"):
            text = subprocess.run(["git", "show", f"{parent}:{name}"], cwd=ROOT, check=True, capture_output=True, text=True).stdout
            with open(os.path.join(directory, os.path.basename(name)), "w") as f:
                f.write("" if name.endswith("__init__.py") else text)   # (the package's __init__ loads more than the wrapper)
    return directory, commit


def forms(env):
    mv, codes = W.Duck((N, 4), W.I32), W.Duck((N, 5, 11, 11), W.U8)
    views, v_attrs, e_attrs = W.Duck((N, 4, 16, 11, 11), W.F16), W.Duck((N, 4, 12), W.I32), W.Duck((N, 4), W.I32)
    return (("step_device", lambda: env.step_device(mv)),
            ("step_device_range, moves only", lambda: env.step_device_range(0, 16384, mv, 0x77)),
            ("step_device_range, with codes", lambda: env.step_device_range(0, 16384, mv, 0x77, codes)),
            ("step_device_range, fogged views, both attribute arrays",
             lambda: env.step_device_range(0, 16384, mv, 0x77, planes=views, view_radius=4, viewer_attrs=v_attrs, env_attrs=e_attrs)),
            ("step_device_range, raw addresses", lambda: env.step_device_range(0, 16384, 0x1000, 0x77, 0x2000)))


def us_per_call(fn, calls: int) -> float:
    t0 = time.perf_counter_ns()
    for _ in range(calls):
        fn()
    return (time.perf_counter_ns() - t0) / calls / 1e3


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent", default="HEAD^")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20000)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as scratch:
        directory, label = parent_package(a.parent, scratch)
        parent = W.load_scratch_package(directory)
    from pomcpp_amd import batch as branch
    sides = [(side, forms(W.handle(mod.BatchEnvironment, Nothing(), n=N))) for side, mod in (("parent", parent), ("branch", branch))]
    for _, fs in sides:   # warm both up
        for _, fn in fs:
            us_per_call(fn, 2000)
    us = {(side, name): [] for side, fs in sides for name, _ in fs}
    gc.disable()
    for _ in range(a.runs):
        for i in range(len(sides[0][1])):
            for side, fs in sides:   # parent and branch alternate, form by form
                us[side, fs[i][0]].append(us_per_call(fs[i][1], a.calls))
    gc.enable()
    print(f"us per call under a do-nothing library, {a.runs} runs of {a.calls} calls, parent ({label}) and branch alternating")
    print(f"{'form':56s} {'parent median':>13s} {'spread':>7s} {'min':>6s} {'branch median':>13s} {'spread':>7s} {'min':>6s}  rule")
    failed = 0
    for name, _ in sides[0][1]:
        p, b = us["parent", name], us["branch", name]
        ok = statistics.median(b) <= statistics.median(p) + (max(p) - min(p))
        failed += not ok
        print(f"{name:56s} {statistics.median(p):13.2f} {max(p) - min(p):7.2f} {min(p):6.2f} {statistics.median(b):13.2f} {max(b) - min(b):7.2f} {min(b):6.2f}  "
              f"{'ok' if ok else 'SLOWER'}")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
