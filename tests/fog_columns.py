"""TEST INFRASTRUCTURE — where the hand-made cases of the fog calls (tests/imagine_cases.py, tests/view_memory_cases.py) sit in a batch
when they are run through the kernels, and what a set of such placements covers.  The kernels work on tiles of 16 envs, four lanes an
env: pom_imagine_kernel stages the views of columns 0..7 and 8..15 in two halves, pom_view_memory_kernel runs one wavefront per pass of
four columns, and the batch's last tile may be short.  A case that only ever sat in column 0 has not met any of that, so the GPU tests
rotate the cases through the columns and the checks below recount, from the placements alone, that every case has been everywhere —
the idea of test_compositions_cover_what_they_claim in tests/test_tile_mates.py.  Plain functions, no GPU."""
import numpy as np

FILLER = -1   # a slot that holds no case: the stated filler State (view memory), or "no job" (imagine)


def slots(n_cases, r):
    """the env slot of each case when they sit side by side from slot r on: case i in slot i + r, tile column (i + r) % 16; every other
    slot of the batch holds the filler"""
    return np.arange(n_cases) + r


def jobs(n_cases, r, count):
    """the case of each job of a call of `count` jobs that repeats the cases with rotation r: job j builds case (j + r) % n_cases, so
    the tile-mates of a case are the other cases"""
    return (np.arange(count) + r) % n_cases


def cases_of_slots(n_cases, r, n):
    """slots() seen from the batch: the case in each of the n env slots, FILLER where there is none"""
    out = np.full(n, FILLER, dtype=np.int64)
    at = slots(n_cases, r)
    assert at[-1] < n, (n_cases, r, n)
    out[at] = np.arange(n_cases)
    return out


def columns(case_of_env, n_cases, first=0):
    """[{tile columns}] per case of one placement: case_of_env[k] is the case in env first + k"""
    out = [set() for _ in range(n_cases)]
    for k, c in enumerate(case_of_env):
        if c != FILLER:
            out[int(c)].add((first + k) % 16)
    return out


def covered(placements, n_cases):
    """the union of columns() over [(case_of_env, first)]"""
    out = [set() for _ in range(n_cases)]
    for case_of_env, first in placements:
        for have, more in zip(out, columns(case_of_env, n_cases, first)):
            have |= more
    return out


def check_columns(placements, n_cases):
    """every case occupies each of the 16 columns — so both staging halves of imagine (column / 8) and all four passes of the view
    memory (column / 4), said once more by name"""
    for i, cols in enumerate(covered(placements, n_cases)):
        assert cols == set(range(16)), (i, sorted(set(range(16)) - cols))
        assert {c // 8 for c in cols} == {0, 1} and {c // 4 for c in cols} == {0, 1, 2, 3}, i


def in_short_tile(placements, n):
    """the cases that some placement puts into the batch's short last tile (n % 16 envs), with the columns they take there"""
    assert n % 16, n
    out = {}
    for case_of_env, first in placements:
        for k, c in enumerate(case_of_env):
            if c != FILLER and first + k >= n - n % 16:
                out.setdefault(int(c), set()).add((first + k) % 16)
    return out


def stacked_rows(views, reverse):
    """the view row of each case in a memory that stacks the cases' one-env memories along the env axis, as listed or reversed: case i
    is env i (reversed: n - 1 - i), its view row 4 * env + views[i]"""
    n = len(views)
    env = np.arange(n)[::-1] if reverse else np.arange(n)
    return 4 * env + np.asarray(views)
