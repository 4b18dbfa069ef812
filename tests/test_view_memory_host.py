"""pom_batch_remember_view (include/pom_batch.h PomMemorySpec) without a GPU: the checker (tests/view_memory_oracle.py) leaves the
bytes reasoned by hand on the hand-made cases (tests/view_memory_cases.py); the kernel's rule functions compiled for the host
(tests/emul/pom_view_memory_emul.cpp) equal the checker on those cases and on a batch of SimpleAgent games played by the CPU oracle —
which is asserted to exercise every clause of the rule —; the wrapper's refusals and spec; the header's struct."""
import ctypes as C
import importlib.util
import os
import sys

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, _MemorySpec
from tests import view_memory_cases as VC
from tests import view_memory_oracle as VM
from tests import wrapper_standin as W
from tests.host_build import ROOT, header_constant, shared_lib, syntax_check
from tests.wrapper_standin import Duck

RADII, MASKS = (0, 1, 4, 10), (1, 0b1010, 15)


@pytest.fixture(scope="module")
def obs():
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def emul():
    """the kernel's rule functions (pomcpp_amd/csrc/pom_view_memory.h) built for the host"""
    lib = C.CDLL(shared_lib("tests/emul/pom_view_memory_emul.cpp"))
    lib.pom_emul_remember.argtypes = [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6

    def run(memory, stamp, codes, agent_attrs, env_attrs, episodes, radius, mask=15):
        """one call on the whole batch, in place, as VM.remember"""
        codes, attrs = np.ascontiguousarray(codes, dtype=np.uint8), np.ascontiguousarray(agent_attrs, dtype=np.int32)
        t, ep = np.ascontiguousarray(env_attrs[:, 0], dtype=np.int32), np.ascontiguousarray(episodes, dtype=np.uint32)
        assert memory.flags["C_CONTIGUOUS"] and stamp.flags["C_CONTIGUOUS"] and memory.dtype == np.uint8 and stamp.dtype == np.int32
        assert lib.pom_emul_remember(len(codes), radius, mask, memory.ctypes.data, stamp.ctypes.data, codes.ctypes.data, attrs.ctypes.data,
                                     t.ctypes.data, ep.ctypes.data) == 0
    return run


def _fresh(n, mask):
    """a wiped pair with a sentinel in the views and stamp rows outside the mask"""
    memory, stamp = VM.new_memory(n)
    for v in range(4):
        if not (mask >> v) & 1:
            memory[:, v], stamp[:, v] = 0xEE, 0x5EED
    return memory, stamp


CASES = VC.cases()


def test_the_cases_cover_every_clause():
    assert {c["name"] for c in CASES} >= {
        "bomb_runs_out_unseen", "bomb_runs_out_under_agent", "flame_runs_out", "enemy_remembered_seen_elsewhere_dead", "own_trail_radius_0",
        "dead_viewer", "age_saturates_never_seen_stays", "wipe_on_new_episode", "wipe_on_earlier_time_step", "dt_0", "dt_3",
        "window_clipped_at_a_corner"}
    assert all(2 <= len(c["frames"]) <= 5 and c["expect"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_checker_leaves_the_bytes_reasoned_by_hand_and_the_host_build_equals_it(obs, emul, case):
    memory, stamp = _fresh(1, case["mask"])
    mine, my_stamp = memory.copy(), stamp.copy()
    shots = []
    for state, episode in case["frames"]:
        inp = VC.inputs_of(obs, state, episode)
        VM.remember(memory, stamp, *inp, case["radius"], case["mask"])
        emul(mine, my_stamp, *inp, case["radius"], case["mask"])
        assert np.array_equal(mine, memory), np.argwhere(mine != memory)[:5]
        assert np.array_equal(my_stamp, stamp)
        shots.append(memory[0].copy())
        for v in range(4):
            want = [episode, int(state["timeStep"][0])] if (case["mask"] >> v) & 1 else [0x5EED, 0x5EED]
            assert stamp[0, v].tolist() == want
    for k, v, x, y, six in case["expect"]:
        assert shots[k][v, :, y, x].tolist() == six, (case["name"], k, v, x, y, shots[k][v, :, y, x].tolist(), six)


def test_hand_written_rows(obs):
    """whole views, reasoned from the rule"""
    by = {c["name"]: c for c in CASES}

    def play(name):
        c = by[name]
        memory, stamp = _fresh(1, c["mask"])
        for state, episode in c["frames"]:
            VM.remember(memory, stamp, *VC.inputs_of(obs, state, episode), c["radius"], c["mask"])
        return memory[0]
    # radius 0, three steps to the right from (4, 4): three cells were ever seen, the age plane reads 2, 1, 0 along the trail
    m = play("own_trail_radius_0")[0]
    assert (m[5] != 255).sum() == 3 and m[5, 4, 4:7].tolist() == [2, 1, 0] and m[0, 4, 4:7].tolist() == [0, 0, 10]
    assert (m[0] == 5).sum() == 118 and not m[1:5].any()
    # two corners at radius 4: 25 cells each with age 0, the other 96 never seen; the views outside the mask keep the sentinel
    m = play("window_clipped_at_a_corner")
    for v, rows in ((0, slice(0, 5)), (3, slice(6, 11))):
        assert (m[v, 5] == 0).sum() == 25 and (m[v, 5] == 255).sum() == 96 and (m[v, 5, rows, rows] == 0).all()
        assert (m[v, 0] == 5).sum() == 96 and (m[v, 0, rows, rows] != 5).all()
    assert (m[1] == 0xEE).all() and (m[2] == 0xEE).all()
    # a new episode: nothing of the old game is left — only the new window, nine cells, is not fog
    m = play("wipe_on_new_episode")[0]
    assert (m[0] != 5).sum() == 9 and (m[5] == 0).sum() == 9 and (m[5] == 255).sum() == 112
    # the saturated age: one cell at 254, one at 0, the rest never seen
    m = play("age_saturates_never_seen_stays")[0]
    assert sorted(m[5].reshape(-1).tolist())[:3] == [0, 254, 255] and (m[5] == 255).sum() == 119


# ---- a batch played on the CPU ------------------------------------------------------------------------------------------------------
N_GAMES, TICKS, CAP, SEED, BSEED = 40, 40, 30, 20261020, 11


@pytest.fixture(scope="module")
def played(oracle, obs):
    """SimpleAgent x4 on N_GAMES generated boards, TICKS ticks, a fresh board after every game (at most CAP ticks long): per tick
    (codes, agent_attrs, env_attrs, episodes).  Computed once, shared, never changed."""
    n = N_GAMES
    states = oracle.boardgen(BSEED, np.arange(n), np.zeros(n))
    eps, mems = np.zeros(n, dtype=np.int32), np.zeros((n, 4, 16), dtype=np.int32)
    frames = []
    for tick in range(TICKS + 1):
        _, attrs, env2 = obs.observe(states)
        env = np.zeros((n, 4), dtype=np.int32)
        env[:, :2] = env2
        frames.append((obs.observe_codes(states), attrs, env, eps.astype(np.uint32)))
        oracle.run_simple_fresh(states, eps, mems, 1, SEED, BSEED, 0, tick, CAP)
    for f in frames:
        for a in f:
            a.setflags(write=False)
    return frames


@pytest.mark.parametrize("radius", RADII)
def test_host_build_equals_the_checker_on_played_games(played, emul, radius):
    totals = dict.fromkeys(VM.COUNTS, 0)
    for mask in MASKS:
        memory, stamp = _fresh(N_GAMES, mask)
        mine, my_stamp = memory.copy(), stamp.copy()
        for tick, inp in enumerate(played):
            counts = VM.remember(memory, stamp, *inp, radius, mask)
            emul(mine, my_stamp, *inp, radius, mask)
            bad = np.argwhere(mine != memory)
            assert bad.size == 0, (mask, tick, bad[:5])
            assert np.array_equal(my_stamp, stamp), (mask, tick)
            for k in totals:
                totals[k] += counts[k]
        for v in range(4):
            if not (mask >> v) & 1:
                assert (memory[:, v] == 0xEE).all() and (stamp[:, v] == 0x5EED).all()
        if radius == 10:   # nothing is fogged: the code planes with age 0
            v = (mask & -mask).bit_length() - 1
            assert np.array_equal(memory[:, v, :5], played[-1][0]) and not memory[:, v, 5].any()
    # The batch exercises the rule: every clause fires where the radius lets it.  Radius 10 has no outside: only the wipes are left.
    # Radius 0 shows the viewer its own cell alone: its own bombs (planted under it) and its own trail, never a flame or another agent.
    must = {0: ("wipes", "expired_bombs", "cleared_seen_elsewhere"), 1: VM.COUNTS, 4: VM.COUNTS, 10: ("wipes",)}[radius]
    assert all(totals[k] > 0 for k in must), (totals, must)


def test_every_kth_tick_ages_by_k_and_a_repeat_changes_nothing(played, emul):
    memory, stamp = _fresh(N_GAMES, 15)
    mine, my_stamp = memory.copy(), stamp.copy()
    for tick in range(0, TICKS + 1, 3):
        VM.remember(memory, stamp, *played[tick], 4)
        emul(mine, my_stamp, *played[tick], 4)
        assert np.array_equal(mine, memory) and np.array_equal(my_stamp, stamp), tick
        again, again_stamp = mine.copy(), my_stamp.copy()
        emul(again, again_stamp, *played[tick], 4)
        assert np.array_equal(again, mine) and np.array_equal(again_stamp, my_stamp), tick
    ages = memory[:, :, 5]
    assert set(np.unique(ages[(ages != 255)]).tolist()) <= set(range(0, 255, 3)) and (ages == 3).any()


# ---- the wrapper: refusals before any library call, in the style of tests/test_wrapper_args_host.py --------------------------------
N, U8, I32 = W.N, W.U8, W.I32


def _pair():
    return Duck((N, 4, 6, 11, 11), U8), Duck((N, 4, 2), I32)


def test_wrapper_refuses_bad_arguments_before_any_library_call(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = W.handle(BatchEnvironment)
    rows = [(dict(view_radius=-1), "view_radius"), (dict(view_radius=11), "view_radius"), (dict(agents=[]), "agents"), (dict(agents=0), "agents"),
            (dict(agents=16), "agents"), (dict(agents=[4]), "agents"), (dict(first=-16), "outside the batch"), (dict(first=16, count=N), "outside the batch"),
            (dict(first=0, count=N + 1), "outside the batch"), (dict(count=-1), "outside the batch"),
            (dict(viewer_attrs=Duck((N, 4, 8), I32)), "viewer_attrs"), (dict(env_attrs=Duck((N, 4), U8)), "env_attrs")]
    for bad in (Duck((N, 4, 5, 11, 11), U8), Duck((N, 4, 6, 11, 11), I32), Duck((N - 4, 4, 6, 11, 11), U8), Duck((N, 4, 6, 121), U8),
                Duck((N, 4, 6, 11, 11), U8, contiguous=False), Duck((N, 4, 6, 11, 11), U8, device="cpu"), None):
        rows.append((dict(memory=bad), "memory"))
    for bad in (Duck((N, 4), I32), Duck((N, 4, 2), "torch.int64"), Duck((N, 4, 2), I32, contiguous=False), None):
        rows.append((dict(stamp=bad), "stamp"))
    for kw, named in rows:
        memory, stamp = _pair()
        args = dict(memory=memory, stamp=stamp)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            env.remember(**args)
        assert named in str(e.value), (kw, str(e.value))
        assert not env._lib.calls, (kw, env._lib.calls)
    assert len(rows) == 12 + 7 + 4


def test_wrapper_builds_the_spec(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = W.handle(BatchEnvironment)

    def spec_of(*a, **kw):
        env.remember(*a, **kw)
        (entry, args), = env._lib.calls
        env._lib.calls.clear()
        assert entry == "pom_batch_remember_view" and isinstance(args[3]._obj, _MemorySpec)
        s = args[3]._obj
        assert s.struct_size == C.sizeof(_MemorySpec) == 48 and s.reserved_ == 0
        return args[1], args[2], s, args[4]
    memory, stamp = _pair()
    first, count, s, stream = spec_of(memory, stamp)
    assert (first, count, stream) == (0, N, None)
    assert (s.view_radius, s.agent_mask, s.memory_dev, s.stamp_dev, s.viewer_attrs_dev, s.env_attrs_dev) == (4, 15, memory.address, stamp.address, None, None)
    va, ea = Duck((N, 4, 12), I32), Duck((N, 4), I32)
    first, count, s, stream = spec_of(memory, stamp, 0, [1, 3], 16, None, W.SimpleNamespace(cuda_stream=0x77), va, ea)
    assert (first, count, stream) == (16, N - 16, 0x77)
    assert (s.view_radius, s.agent_mask, s.viewer_attrs_dev, s.env_attrs_dev) == (0, 0b1010, va.address, ea.address)
    first, count, s, stream = spec_of(0x1000, 0x2000, view_radius=10, agents=1, first=0, count=16, stream=0x99)   # raw addresses pass unchecked
    assert (first, count, stream, s.memory_dev, s.stamp_dev, s.view_radius, s.agent_mask) == (0, 16, 0x99, 0x1000, 0x2000, 10, 1)


def test_new_view_memory_is_a_wiped_pair():
    """(on the CPU: torch only owns the memory)"""
    memory, stamp = pa.new_view_memory(3, "cpu")
    want_m, want_s = VM.new_memory(3)
    assert memory.dtype.is_floating_point is False and tuple(memory.shape) == (3, 4, 6, 11, 11) and tuple(stamp.shape) == (3, 4, 2)
    assert np.array_equal(memory.numpy(), want_m) and np.array_equal(stamp.numpy(), want_s)


# ---- the header -----------------------------------------------------------------------------------------------------------------
SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomMemorySpec) == POM_MEMORY_SPEC_SIZE ? 1 : -1];
typedef char offsets[offsetof(PomMemorySpec, view_radius) == 4 && offsetof(PomMemorySpec, agent_mask) == 8 && offsetof(PomMemorySpec, reserved_) == 12 &&
                     offsetof(PomMemorySpec, memory_dev) == 16 && offsetof(PomMemorySpec, stamp_dev) == 24 &&
                     offsetof(PomMemorySpec, viewer_attrs_dev) == 32 && offsetof(PomMemorySpec, env_attrs_dev) == 40 ? 1 : -1];
int use(PomBatch* h, void* stream)
{
    PomMemorySpec s = {sizeof(PomMemorySpec), 4, 15, 0, 0, 0, 0, 0};
    return pom_batch_remember_view(h, 0, 16, &s, stream);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert header_constant("POM_MEMORY_SPEC_SIZE") == 48 == C.sizeof(_MemorySpec)
    assert header_constant("POM_MEMORY_PLANES") == 6 == pa.batch.MEMORY_PLANES == VM.PLANES


def test_header_struct_equals_the_ctypes_struct(tmp_path):
    from tests.test_abi_mirror import layout_differences
    assert layout_differences({"PomMemorySpec": _MemorySpec}, tmp_path) == []
