"""TEST INFRASTRUCTURE — the checker of pom_batch_expand (include/pom_batch.h PomExpandSpec): what the batch and the result words must
be after env first + j became the successor of env src[j] under moves[j].  The tick is the CPU checker's (Oracle.step for POM_MODE_RAW,
Oracle.env_step for POM_MODE_ENV) on a copy of the source; the no-job rules and the result word are restated here from the header."""
import numpy as np

MODE_RAW, MODE_ENV = 0, 1
RO_NONE, RO_DONE, RO_DRAW, RO_TIMEOUT, RO_UB, RO_WINNER_SHIFT, RO_LENGTH_SHIFT = 0, 0x10, 0x20, 0x40, 0x80, 8, 16


def blank_status(n):
    """the statuses of n freshly uploaded envs"""
    return dict(done=np.zeros(n, dtype=np.int32), winner=np.full(n, -1, dtype=np.int32), draw=np.zeros(n, dtype=np.int32),
                timeout=np.zeros(n, dtype=np.int32), ubflags=np.zeros(n, dtype=np.uint32))


def is_job(s, d, first, count, n):
    """the header's rule: a source of the batch that is not another slot of the range"""
    return 0 <= s < n and not (first <= s < first + count and s != d)


def word(state, status, e, ub, length):
    alive = sum((0 if state["agents"]["dead"][e][a] else 1) << a for a in range(4))
    return (alive | (RO_DONE if status["done"][e] else 0) | (RO_DRAW if status["draw"][e] else 0) | (RO_TIMEOUT if status["timeout"][e] else 0) |
            (RO_UB if ub else 0) | (int(status["winner"][e]) + 1) << RO_WINNER_SHIFT | length << RO_LENGTH_SHIFT)


def expand(oracle, states, status, src, moves, first, mode, max_steps=0):
    """states: STATE_DTYPE [n]; status: blank_status' arrays (None: blank); src int64 [count]; moves int32 [count, 4].
    Returns (states, status, words uint32 [count], ticks played, children newly done) — new arrays, the inputs are not written."""
    n, count = states.size, len(src)
    assert 0 <= first and first + count <= n and np.asarray(moves).shape == (count, 4)
    status = blank_status(n) if status is None else status
    out, st = states.copy(), {k: v.copy() for k, v in status.items()}
    words = np.zeros(count, dtype=np.uint32)
    ticks = newly_done = 0
    for j in range(count):
        s, d = int(src[j]), first + j
        if not is_job(s, d, first, count, n):
            continue                                   # env d bit for bit as it was, word POM_RO_NONE
        child = states[s:s + 1].copy()                 # the source as it was BEFORE the call
        cs = {k: int(status[k][s]) for k in status}
        ub, length = 0, 0
        if mode == MODE_RAW:
            ub, length = oracle.step(child, moves[j]), 1
        elif not cs["done"]:                           # a finished source gives an unticked copy
            ub, length = oracle.env_step(child, moves[j], cs), 1
            if max_steps > 0 and int(child["timeStep"][0]) >= max_steps:
                cs["done"] = cs["timeout"] = 1
            newly_done += 1 if cs["done"] else 0
        ticks += length
        cs["ubflags"] |= ub
        child["agents"]["pad"] = 0
        out[d] = child[0]
        for k in st:
            st[k][d] = cs[k]
        words[j] = word(out, st, d, ub != 0, length)
    return out, st, words, ticks, newly_done
