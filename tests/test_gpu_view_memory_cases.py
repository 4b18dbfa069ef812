"""The hand-made cases of pom_batch_remember_view (tests/view_memory_cases.py) through pom_view_memory_kernel itself, in every tile
column.  The host suite runs them one env at a time through the rule functions; the kernel packs a view's dt and wipe into one register
and reads it back by readlane(4 * env + view), loads an env ahead, and runs four wavefronts per tile, one per pass of four envs — and on
the GPU it has only met SimpleAgent games in lockstep: dt 0, 1 or 3, ages below 200.  Here the cases sit side by side in a batch of 45
envs (its last tile has 13, so that tile's fourth pass holds one env) among different mid-game States, rotated through the columns
(tests/fog_columns.py), every frame of every case is uploaded in turn, and the whole memory and stamp tensors are compared with the
checker (tests/view_memory_oracle.py) after every call, as are the bytes the cases reason by hand.  One more call gives every view of
every env another (dt, wipe) head over a memory with ages and lives at their limits."""
import importlib.util
import os

import numpy as np
import pytest

from tests import fog_columns as FC
from tests import view_memory_cases as VC
from tests import view_memory_oracle as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = VC.cases()
C = len(CASES)
N, SEED, BSEED = 45, 20261020, 11
ROTATIONS = list(range(16)) + [31, N - C]   # the last ones reach into the short tile and fill it to the batch's end
RADII = sorted({c["radius"] for c in CASES})
FRAMES = max(len(c["frames"]) for c in CASES)
SENTINEL, SENTINEL_STAMP = 0xEE, 0x5EED
DELTAS = (0, 1, 2, 254, 255, 256, 300, 1000)
gpu = pytest.mark.gpu


# ---- what the placements cover: recounted from the arrays, no GPU ------------------------------------------------------------------
def test_the_rotations_put_every_case_into_every_column_and_into_the_short_tile():
    placements = [(FC.cases_of_slots(C, r, N), 0) for r in ROTATIONS]
    FC.check_columns(placements[:16], C)
    short = FC.in_short_tile(placements, N)
    assert N % 16 == 13 and ROTATIONS[-1] + C == N and set(short) == set(range(C))
    assert any(12 in cols for cols in short.values())   # the one env of the short tile's fourth pass
    assert RADII == [0, 1, 2, 4] and 2 <= FRAMES <= 5


def _delta_index(e, v):
    """which of DELTAS view v of env e is stamped with: the four views of an env differ, and so do the 16 envs of a tile"""
    ec = e % 16
    return (5 * ec + v * (1 + ec // 8)) % len(DELTAS)


def test_the_heads_differ_from_lane_to_lane():
    rows = [tuple(_delta_index(e, v) for v in range(4)) for e in range(16)]
    assert len(set(rows)) == 16 and all(len(set(r)) == 4 for r in rows)
    assert {i for r in rows for i in r} == set(range(len(DELTAS)))


# ---- the GPU ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def obs():
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _inputs(obs, states):
    """what the checker takes of States, from the CPU oracle of the export: (codes, agent_attrs, env_attrs)"""
    _, attrs, env2 = obs.observe(states)
    env = np.zeros((len(states), 4), dtype=np.int32)
    env[:, :2] = env2
    return obs.observe_codes(states), attrs, env


class Stage:
    """the filler — N different States of SimpleAgent games after 12 ticks, played by the CPU oracle — and every frame of every case, with
    the checker's inputs for each.  Made once, shared, never changed."""

    def __init__(self, oracle, obs):
        import pomcpp_amd as pa
        start = pa.make_boards(N, seed=BSEED)
        self.filler = start.copy()
        oracle.run_simple(self.filler, start, np.zeros((N, 4, 16), dtype=np.int32), 12, SEED, 0, 0, 0)
        assert len({s.tobytes() for s in self.filler}) == N and (self.filler["timeStep"] == 12).all()
        self.filler_in = _inputs(obs, self.filler)
        self.frames = [np.concatenate([f[0] for f in c["frames"]]) for c in CASES]
        self.frames_in = [_inputs(obs, f) for f in self.frames]
        self.episodes = [[f[1] for f in c["frames"]] for c in CASES]

    def batch(self, r, k):
        """frame k of every case in its slot of rotation r, the filler elsewhere: (States [N], the checker's inputs, the slots whose case
        starts a new episode with this frame).  A case with fewer frames keeps its last one."""
        states, inp = self.filler.copy(), [a.copy() for a in self.filler_in]
        new_episode = []
        for i, slot in enumerate(FC.slots(C, r)):
            kk = min(k, len(self.frames[i]) - 1)
            states[slot] = self.frames[i][kk]
            for a, b in zip(inp, self.frames_in[i]):
                a[slot] = b[kk]
            if 1 <= k == kk and self.episodes[i][k] != self.episodes[i][k - 1]:
                new_episode.append(int(slot))
        return states, inp, new_episode


@pytest.fixture(scope="module")
def stage(oracle, obs):
    return Stage(oracle, obs)


def _pair(n, mask):
    """a wiped pair on the device and its twin on the host, the views and stamp rows outside the mask holding a sentinel (as _pair() of
    tests/test_view_memory.py)"""
    import torch
    import pomcpp_amd as pa
    memory, stamp = pa.new_view_memory(n)
    want_m, want_s = VM.new_memory(n)
    for v in range(4):
        if not (mask >> v) & 1:
            memory[:, v], stamp[:, v] = SENTINEL, SENTINEL_STAMP
            want_m[:, v], want_s[:, v] = SENTINEL, SENTINEL_STAMP
    torch.cuda.synchronize()
    return memory, stamp, want_m, want_s


def _same(memory, stamp, want_m, want_s, what):
    got = memory.cpu().numpy()
    bad = np.argwhere(got != want_m)
    assert bad.size == 0, f"{what}: memory differs in {len(bad)} bytes, first (env, view, plane, y, x) {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want_m[tuple(bad[0])]}"
    got_s = stamp.cpu().numpy()
    assert np.array_equal(got_s, want_s), f"{what}: stamps differ at (env, view, field) {np.argwhere(got_s != want_s)[:4].tolist()}"
    return got


def _walk(env, stage, r, radius, mask):
    """every frame in turn: upload, realise the frame's episode number in the stamps, call, compare everything"""
    import torch
    memory, stamp, want_m, want_s = _pair(N, mask)
    at = FC.slots(C, r)
    for k in range(FRAMES):
        what = f"rotation {r}, radius {radius}, mask {mask:#x}, frame {k}"
        states, inp, new_episode = stage.batch(r, k)
        env.make_game(states)
        episodes = env.episodes()
        assert not episodes.any()   # (no auto-reset, and an uploaded State is episode 0 of its env)
        if new_episode:
            # the handle's counters cannot be moved from outside: a new game is a stamp whose episode differs from the counter; -1 stays -1
            for slot in new_episode:
                for v in range(4):
                    if (mask >> v) & 1 and want_s[slot, v, 0] != -1:
                        want_s[slot, v, 0] = int(episodes[slot]) + 1
            stamp.copy_(torch.from_numpy(want_s))   # (equal to the device's but for those fields: _same below has just said so)
            torch.cuda.synchronize()
        env.remember(memory, stamp, radius, mask)
        env.sync()
        VM.remember(want_m, want_s, *inp, episodes, radius, mask)
        got = _same(memory, stamp, want_m, want_s, what)
        for v in range(4):
            if not (mask >> v) & 1:
                assert (got[:, v] == SENTINEL).all() and (want_s[:, v] == SENTINEL_STAMP).all(), what
        for i, case in enumerate(CASES):   # the bytes reasoned by hand: views are merged one by one, so a view of both masks is the case's
            if case["radius"] != radius:
                continue
            for kk, v, x, y, six in case["expect"]:
                if kk == k and (case["mask"] >> v) & 1 and (mask >> v) & 1:
                    assert got[at[i], v, :, y, x].tolist() == six, (what, case["name"], v, x, y, got[at[i], v, :, y, x].tolist(), six)


@pytest.fixture(scope="module")
def handle(hip_lib):
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_OFF
    env = BatchEnvironment(N, mode=MODE_ENV, auto_reset=RESET_OFF)
    yield env
    env.close()


@gpu
@pytest.mark.parametrize("r", ROTATIONS)
def test_every_case_in_every_column(handle, stage, r):
    for radius in RADII:
        _walk(handle, stage, r, radius, 15)
    _walk(handle, stage, r, RADII[r % len(RADII)], 0b1010)


def _limit_memory(n):
    """a memory whose every view holds, in cell order from a start that moves with the view, every pairing of the ages 0, 1, 253, 254, 255
    with: passage, rigid, wood, a power-up, bombs and agents on bombs with life 1, 2, 254, 255, agents, flames with life 1, 2, 254, 255
    and a burnt-out flame"""
    lives = (1, 2, 254, 255)
    contents = [(0, 0, 0, 0, 0), (1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (6, 0, 0, 0, 0), (4, 0, 0, 0, 0)]
    contents += [(3, 2, life, 1 + k, 0) for k, life in enumerate(lives)] + [(10 + k, 3, life, 0, 0) for k, life in enumerate(lives)]
    contents += [(10 + k, 0, 0, 0, 0) for k in range(4)] + [(4, 0, 0, 0, life) for life in lives]
    patterns = np.array([c + (age,) for age in (0, 1, 253, 254, 255) for c in contents], dtype=np.uint8)
    assert len(patterns) == 105
    lane = np.arange(4 * n)[:, None]
    memory = patterns[(np.arange(121)[None, :] + 17 * lane) % len(patterns)]   # [4 n, 121, 6]
    return np.ascontiguousarray(memory.transpose(0, 2, 1)).reshape(n, 4, 6, 11, 11)


@gpu
def test_another_head_in_every_lane(hip_lib, obs):
    """One call, radius 1, in which every view of every env has another stamp — t0 = t - DELTAS by _delta_index, and in every tile one view
    of another episode, one with no memory yet and one stamped later than now — over _limit_memory().  A wrong readlane index, or a dt
    that spills into the wipe bit, shows here."""
    import torch
    from pomcpp_amd.batch import BatchEnvironment, MODE_ENV, RESET_AT_END
    with BatchEnvironment(N, mode=MODE_ENV, auto_reset=RESET_AT_END, max_steps=30, fresh_boards=True, board_seed=BSEED) as env:
        env.generate(BSEED)
        env.step_simple(SEED, 75)
        states, episodes = env.get_state(), env.episodes()
        assert (episodes >= 2).all() and len(set(states["timeStep"].tolist())) > 1
        inp = _inputs(obs, states)
        t = inp[2][:, 0].astype(np.int64)
        want_m = _limit_memory(N)
        want_s = np.zeros((N, 4, 2), dtype=np.int32)
        for e in range(N):
            for v in range(4):
                want_s[e, v] = (np.int64(episodes[e]).astype(np.int32), t[e] - DELTAS[_delta_index(e, v)])
            if e % 16 == 3:
                want_s[e, 2, 0] -= 1           # another episode
            if e % 16 == 7:
                want_s[e, 1, 0] = -1           # no memory yet
            if e % 16 == 11:
                want_s[e, 3, 1] = t[e] + 5     # stamped later than now
        heads = {(min(int(t[e] - want_s[e, v, 1]), 255), int(want_s[e, v, 0] != episodes[e] or t[e] < want_s[e, v, 1])) for e in range(16, 32) for v in range(4)}
        assert {(0, 0), (1, 0), (2, 0), (254, 0), (255, 0)} <= heads and any(w for _, w in heads)
        wiped = (want_s[:, :, 0] != episodes.astype(np.int64)[:, None]) | (t[:, None] < want_s[:, :, 1])
        memory, stamp = torch.from_numpy(want_m.copy()).cuda(), torch.from_numpy(want_s.copy()).cuda()
        torch.cuda.synchronize()
        before = want_m.copy()
        env.remember(memory, stamp, 1)
        env.sync()
        counts = VM.remember(want_m, want_s, *inp, episodes, 1)
        got = _same(memory, stamp, want_m, want_s, "another head in every lane")
        assert counts["wipes"] == 3 * 2 and counts["expired_bombs"] and counts["expired_flames"] and counts["cleared_dead"] + counts["cleared_seen_elsewhere"]
        # the limits were met outside the windows: a life of 255 that dt = 255 ends and a life of 255 that dt = 254 leaves at 1, ages that
        # stop at 254, and never-seen cells that stay as they are
        kept = (before[:, :, 5] == 255) & (got[:, :, 5] == 255) & ~wiped[:, :, None, None]
        assert wiped.sum() == 3 * 3
        assert kept.any() and all(np.array_equal(got[:, :, k][kept], before[:, :, k][kept]) for k in range(6))
        assert ((before[:, :, 2] == 255) & (got[:, :, 2] == 0) & (got[:, :, 5] == 254)).any() and ((before[:, :, 2] == 255) & (got[:, :, 2] == 1)).any()
        assert ((before[:, :, 4] == 255) & (before[:, :, 0] == 4) & (got[:, :, 0] == 0) & (got[:, :, 5] == 254)).any()
        assert ((before[:, :, 5] == 253) & (got[:, :, 5] == 254)).any() and ((before[:, :, 5] == 0) & (got[:, :, 5] == 254)).any()
