"""The SimpleAgent policy at the packed record's limits, pinned by the compiled reference (tests/golden/policy_edges.npz, made by
tests/golden/gen_policy_edges.py from the corpus of tests/policy_edge_states.py).

CPU (unmarked): the fixture reaches what it claims (recounted here in plain numpy from the stored states, without the oracle or the
device code); the policy oracle and the host builds of the device policy body (one-lane floods and the quad-word floods) reproduce
every act() vector, Move and memory; the oracle reproduces every act of the games.
GPU: the games replayed through policy_simple + step_policy (moves and memory every tick) and the fused step_simple (memory every
tick), in the default 16 x 4 shape and the one-lane shapes, against the fixture."""
import ctypes as C
import os

import numpy as np
import pytest

from pomcpp_amd.state import STATE_DTYPE
from tests.edge_states import BOMBCOUNT_MAX, BOMBCOUNT_MIN, MAXBOMBS_MAX
from tests.edge_states import uploadable as _uploadable
from tests.host_build import ROOT, shared_lib
from tests.policy_edge_states import check_memory
from tests.test_policy_fixtures import _replay_on_gpu

FIX = os.path.join(ROOT, "tests", "golden", "policy_edges.npz")


@pytest.fixture(scope="module")
def fx():
    z = np.load(FIX)
    d = {k: z[k] for k in z.files}
    d["st"] = np.ascontiguousarray(d["states"]).view(STATE_DTYPE).reshape(-1)
    d["start"] = np.ascontiguousarray(d["game_start"]).view(STATE_DTYPE).reshape(-1)
    return d


# ---------------------------------------------------------------------------------------------------------------- numpy recount
def _live_bombs(s):
    """(x, y, owner, strength, time) of the bombs IsInDanger walks: count entries from index, wrapping at 20"""
    q = s["bombs_queue"].astype(np.int64) & 0xFFFFFFFF
    out = []
    for k in range(int(s["bombs_count"])):
        w = int(q[(int(s["bombs_index"]) + k) % 20])
        out.append((w & 0xF, (w >> 4) & 0xF, (w >> 8) & 0xF, (w >> 12) & 0xF, (w >> 16) & 0xF))
    return out


def _covering_times(s, x, y):
    return [t for bx, by, _, st, t in _live_bombs(s) if (by == y and abs(bx - x) <= st) or (bx == x and abs(by - y) <= st)]


def _danger(s, x, y):
    ts = _covering_times(s, x, y)
    return min(ts) if ts else 0


def _reach(s, x, y):
    """FillRMap's reach from (x, y): walkable cells are passed, agent cells entered"""
    b = s["board"]
    walk = lambda v: v == 0 or 6 <= v <= 8  # noqa: E731  passage, power-ups
    agent = lambda v: v >= (1 << 24)  # noqa: E731
    seen, front = {(x, y)}, [(x, y)]
    while front:
        nxt = []
        for cx, cy in front:
            for nx, ny in ((cx, cy + 1), (cx, cy - 1), (cx + 1, cy), (cx - 1, cy)):
                if 0 <= nx <= 10 and 0 <= ny <= 10 and (nx, ny) not in seen:
                    v = int(b[ny, nx])
                    if walk(v):
                        seen.add((nx, ny))
                        nxt.append((nx, ny))
                    elif agent(v):
                        seen.add((nx, ny))
        front = nxt
    return seen


def _origin_unreachable_chase(s, i, mem):
    """agent i on (0, 0), not in danger, allowed to bomb, no enemy at 1, an enemy within 7, no loop — and MoveTowardsEnemy's
    target out of reach"""
    a = s["agents"]
    if (int(a["x"][i]), int(a["y"][i])) != (0, 0) or _danger(s, 0, 0) > 0 or not int(a["bombCount"][i]) < int(a["maxBombCount"][i]):
        return False
    enemies = [j for j in range(4) if j != i and not a["dead"][j]]
    dist = lambda j: abs(int(a["x"][j])) + abs(int(a["y"][j]))  # noqa: E731
    if any(dist(j) <= 1 for j in enemies) or not any(dist(j) <= 7 for j in enemies):
        return False
    rp = [(int(mem[2 * ((int(mem[8]) + k) % 4)]), int(mem[2 * ((int(mem[8]) + k) % 4) + 1])) for k in range(4)]
    if all(rp[k] == rp[k + 2] for k in range(int(mem[9]) // 2)):
        return False
    target = next(j for j in range(4) if not a["dead"][j] and (int(a["x"][j]), int(a["y"][j])) != (0, 0) and dist(j) <= 7)
    return (int(a["x"][target]), int(a["y"][target])) not in _reach(s, 0, 0)


def test_fixture_reaches_what_it_claims(fx):
    st, ks, ids = fx["st"], fx["act_state"], fx["act_agent"].astype(int)
    n = ks.size
    assert n > 50000 and st.size > 4000
    counts = dict(timer0=0, spill=0, bombs20_wrapped=0, bc_min=0, bc_max=0, mb_max=0, mb_min=0, origin_unreached=0, stale=0)
    for v in range(n):
        s, i, mem_in, mem_out = st[ks[v]], ids[v], fx["act_mem_in"][v], fx["act_mem_out"][v]
        a = s["agents"]
        x, y = int(a["x"][i]), int(a["y"][i])
        counts["timer0"] += 0 in _covering_times(s, x, y)
        counts["spill"] += any(int(a["bombStrength"][o]) > 15 for _, _, o, _, _ in _live_bombs(s))
        counts["bombs20_wrapped"] += int(s["bombs_count"]) == 20 and int(s["bombs_index"]) != 0
        counts["bc_min"] += int(a["bombCount"][i]) == BOMBCOUNT_MIN
        counts["bc_max"] += int(a["bombCount"][i]) == BOMBCOUNT_MAX
        counts["mb_max"] += int(a["maxBombCount"][i]) == MAXBOMBS_MAX
        counts["mb_min"] += int(a["maxBombCount"][i]) == -32768
        counts["origin_unreached"] += (x, y) == (0, 0) and _origin_unreachable_chase(s, i, mem_in)
        # an odd draw read moveQueue slot 1 past a count of 1: what was there before (it differs from slot 0)
        counts["stale"] += (int(mem_out[15]) == 1 and fx["act_draw"][v] % 2 == 1 and mem_out[11] != mem_out[10]
                            and fx["act_move"][v] == mem_out[11])
        check_memory(mem_in)
        check_memory(mem_out)
    print(counts)
    assert min(counts.values()) >= 8, counts
    # every Move; draw-dependent inputs carry all five draws
    assert (np.bincount(fx["act_move"].astype(int), minlength=6) > 0).all()
    assert set(np.unique(fx["act_draw"]).tolist()) == {0, 1, 2, 3, 4}
    # the game layout: agents in danger on the first tick, per wavefront of 16 env slots
    start = fx["start"]
    jobs = []
    for w in range(0, start.size, 16):
        jobs.append(sum(_danger(s, int(s["agents"]["x"][i]), int(s["agents"]["y"][i])) > 0
                        for s in start[w:w + 16] for i in range(4) if not s["agents"]["dead"][i]))
    assert jobs == fx["game_fwd_jobs"].tolist()
    assert {0, 1, 16, 17, 32, 33, 64} <= set(jobs) and start.size % 16 != 0
    live = np.arange(fx["game_moves"].shape[1])[None, :] < fx["game_length"][:, None]
    assert not fx["game_asked"][~live].any() and fx["game_asked"][live].sum() > 10000


# ---------------------------------------------------------------------------------------------------------------- oracle, host body
def test_oracle_reproduces_every_act_vector(fx, oracle):
    lib = oracle.lib
    st = fx["st"]
    for v in range(fx["act_state"].size):
        mem = fx["act_mem_in"][v].astype(np.int32)
        s = st[fx["act_state"][v]:fx["act_state"][v] + 1]
        got = lib.pom_oracle_simple_act(s.ctypes.data, int(fx["act_agent"][v]), mem.ctypes.data, int(fx["act_draw"][v]))
        assert got == fx["act_move"][v] and np.array_equal(mem, fx["act_mem_out"][v]), (
            f"act {v} ({fx['state_names'][fx['act_state'][v]]}, agent {fx['act_agent'][v]}, draw {fx['act_draw'][v]}): "
            f"oracle {got} {mem.tolist()}, reference {fx['act_move'][v]} {fx['act_mem_out'][v].tolist()}")


def test_oracle_replays_the_games(fx, oracle):
    lib = oracle.lib
    lib.pom_oracle_policy_draw.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_int]
    seed, start, length = int(fx["game_seed"][0]), fx["start"], fx["game_length"]
    for e in range(start.size):
        s = start[e:e + 1].copy()
        mem = np.zeros((4, 16), dtype=np.int32)
        for t in range(int(length[e])):
            mv = np.zeros(4, dtype=np.int32)
            for i in range(4):
                if not fx["game_asked"][e, t, i]:
                    assert s["agents"]["dead"][0, i]
                    continue
                draw = int(fx["game_draws"][e, t, i])
                assert draw == lib.pom_oracle_policy_draw(seed, e, t, i)
                mv[i] = lib.pom_oracle_simple_act(s.ctypes.data, i, mem[i].ctypes.data, draw)
                assert mv[i] == fx["game_moves"][e, t, i] and np.array_equal(mem[i], fx["game_memory"][e, t, i]), (e, t, i)
            oracle.step(s, mv)
            s["timeStep"][0] += 1


@pytest.fixture(scope="module")
def policy_emul():
    lib = C.CDLL(shared_lib("tests/emul/pom_policy_emul.cpp"))
    lib.pom_emul_simple_act.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.pom_emul_simple_act.restype = C.c_int
    return lib


@pytest.mark.parametrize("floods", ["one-lane", "quad"])
def test_device_policy_body_reproduces_every_act_vector(fx, policy_emul, floods):
    """every vector whose state upload accepts (the host build packs the state for each act; a tick can carry a field past its
    upload bound — bombCount 107 + a plant — which the device record then holds but upload refuses: those pin the oracle only)"""
    C.c_int.in_dll(policy_emul, "pom_emul_quad_floods").value = int(floods == "quad")
    st = fx["st"]
    refused = 0
    for v in range(fx["act_state"].size):
        mem = fx["act_mem_in"][v].astype(np.int32)
        s = st[fx["act_state"][v]:fx["act_state"][v] + 1]
        got = policy_emul.pom_emul_simple_act(s.ctypes.data, int(fx["act_agent"][v]), mem.ctypes.data, int(fx["act_draw"][v]))
        if got == -1:
            assert not _uploadable(s[0]), f"act {v}: a state within upload's bounds refused"
            refused += 1
            continue
        assert got == fx["act_move"][v] and np.array_equal(mem, fx["act_mem_out"][v]), (
            f"act {v} ({fx['state_names'][fx['act_state'][v]]}, agent {fx['act_agent'][v]}, draw {fx['act_draw'][v]}): "
            f"device body {got} {mem.tolist()}, reference {fx['act_move'][v]} {fx['act_mem_out'][v].tolist()}")
    assert refused < fx["act_state"].size // 20, refused


# ---------------------------------------------------------------------------------------------------------------- GPU
SHAPES = [{}, dict(lanes_per_env=1, envs_per_wave=16), dict(envs_per_wave=64)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["16x4", "16x1", "64x1"])
@pytest.mark.parametrize("fused", [False, True], ids=["policy_then_step", "step_simple"])
def test_gpu_replays_the_reference_games(hip_lib, fx, shape, fused):
    """117 games in a ragged batch (the last wavefront of 16 holds 5): every Move (two-kernel form) and every agent's memory"""
    assert _replay_on_gpu(fx, fused=fused, **shape) > 10000


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [0xF, 0b0101], ids=["mask_1111", "mask_0101"])
def test_gpu_mixed_step_replays_the_reference_games(hip_lib, fx, mask):
    """the same 117 games through pom_batch_step_mixed: with 0b0101 agents 1 and 3 take the Moves the fixture recorded, so any mask
    must reproduce the same game — the masked agents' memory is the fixture's, the state a step_simple twin's, every tick"""
    assert _replay_on_gpu(fx, via="mixed", mask=mask) > (10000 if mask == 0xF else 5000)


@pytest.mark.gpu
def test_gpu_replays_a_ragged_prefix(hip_lib, fx):
    """the first 16 * 3 + 1 games only: the last wavefront holds one env"""
    sub = dict(fx)
    for k in ("start", "game_length", "game_draws", "game_moves", "game_asked", "game_memory"):
        sub[k] = fx[k][:49]
    assert _replay_on_gpu(sub, fused=False) > 4000
