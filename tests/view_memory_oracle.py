"""TEST INFRASTRUCTURE — THE RULE of pom_batch_remember_view (include/pom_batch.h PomMemorySpec) in plain numpy, from the UNFOGGED
outputs the suite already pins: the code planes (observe(dtype="codes") / oracle/pom_observe_oracle.py observe_codes), agent_attrs,
env_attrs and the episode counters.  The reference has no fog and no memory: this checker is the authority for the call, as
tests/view_oracle.py is for the views.  Nothing of the kernel's own arithmetic is restated: the steps are written as the header
numbers them, on whole arrays."""
import numpy as np

from tests.view_oracle import windows

PLANES, FOG, BOMB, FLAMES, AGENT0, NEVER, AGE_MAX = 6, 5, 3, 4, 10, 255, 254
BOARD, STRENGTH, LIFE, DIR, FLAME, AGE = range(6)
COUNTS = ("expired_bombs", "expired_flames", "cleared_seen_elsewhere", "cleared_dead", "wipes")


def new_memory(n):
    """a wiped (memory uint8 [n, 4, 6, 11, 11], stamp int32 [n, 4, 2]) pair"""
    memory = np.zeros((n, 4, PLANES, 11, 11), dtype=np.uint8)
    memory[:, :, BOARD], memory[:, :, AGE] = FOG, NEVER
    return memory, np.full((n, 4, 2), -1, dtype=np.int32)


def remember(memory, stamp, codes, agent_attrs, env_attrs, episodes, radius, mask=15, first=0, count=None):
    """One call on the envs [first, first + count) and the agents of `mask`, IN PLACE on memory and stamp.  codes uint8 [n, 5, 11, 11],
    agent_attrs int32 [n, 4, 8] (x, y, alive, ...), env_attrs int32 [n, 4] (timeStep first), episodes [n].  Returns how often each
    clause fired, a dict over COUNTS (cells; wipes: views that held a memory and lost it)."""
    n = len(codes)
    count = n - first if count is None else count
    sl = slice(first, first + count)
    counts = dict.fromkeys(COUNTS, 0)
    win = windows(agent_attrs, radius)                          # [n, 4, 11, 11]
    x, y, alive = (agent_attrs[:, :, k].astype(np.int64) for k in (0, 1, 2))
    ep, t = np.asarray(episodes).astype(np.int64), env_attrs[:, 0].astype(np.int64)
    for v in range(4):
        if not (mask >> v) & 1:
            continue
        m = memory[sl, v].astype(np.int64)                      # [c, 6, 11, 11]
        inside = win[sl, v]
        ep0, t0 = stamp[sl, v, 0].astype(np.int64), stamp[sl, v, 1].astype(np.int64)
        # step 1: wipe ...
        wipe = ((ep0 & 0xFFFFFFFF) != (ep[sl] & 0xFFFFFFFF)) | (t[sl] < t0)
        counts["wipes"] += int((wipe & (ep0 != -1)).sum())
        dt = np.where(wipe, 0, np.minimum(t[sl] - t0, 255))[:, None, None]
        # ... or age, outside the window, where something was seen (1.1) and time has passed
        aging = ~inside & ~wipe[:, None, None] & (m[:, AGE] != NEVER) & (dt > 0)
        a = m.copy()
        # 1.2 bombs
        life = np.maximum(a[:, LIFE] - dt, 0)
        out = (a[:, LIFE] > 0) & (life == 0)
        counts["expired_bombs"] += int((out & aging).sum())
        a[:, LIFE] = life
        for k in (STRENGTH, DIR):
            a[:, k][out] = 0
        a[:, BOARD][out & (a[:, BOARD] == BOMB)] = 0
        # 1.3 flames
        fl = a[:, BOARD] == FLAMES
        left = np.maximum(a[:, FLAME] - dt, 0)
        a[:, FLAME] = np.where(fl, left, a[:, FLAME])
        counts["expired_flames"] += int((fl & (left == 0) & aging).sum())
        a[:, BOARD][fl & (left == 0)] = 0
        # 1.4 stale agents: dead, or standing inside this viewer's window now
        for g in range(4):
            here = a[:, BOARD] == AGENT0 + g
            dead = alive[sl, g] == 0
            seen = win[np.arange(first, first + count), v, np.clip(y[sl, g], 0, 10), np.clip(x[sl, g], 0, 10)] & \
                (x[sl, g] <= 10) & (y[sl, g] <= 10)
            gone = (dead | seen)[:, None, None] & here
            counts["cleared_dead"] += int((gone & aging & dead[:, None, None]).sum())
            counts["cleared_seen_elsewhere"] += int((gone & aging & ~dead[:, None, None]).sum())
            a[:, BOARD] = np.where(gone, np.where(a[:, LIFE] > 0, BOMB, 0), a[:, BOARD])
        # 1.5
        a[:, AGE] = np.minimum(a[:, AGE] + dt, AGE_MAX)
        m = np.where(aging[:, None], a, m)
        wiped = np.zeros_like(m)
        wiped[:, BOARD], wiped[:, AGE] = FOG, NEVER
        m = np.where(wipe[:, None, None, None], wiped, m)
        # step 2: the window
        now = np.concatenate([codes[sl].astype(np.int64), np.zeros((count, 1, 11, 11), dtype=np.int64)], axis=1)
        m = np.where(inside[:, None], now, m)
        memory[sl, v] = m.astype(np.uint8)
        # step 3
        stamp[sl, v, 0] = (ep[sl] & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
        stamp[sl, v, 1] = t[sl]
    return counts
