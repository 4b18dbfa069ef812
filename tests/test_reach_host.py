"""pom_batch_reach (include/pom_batch.h PomReachSpec) without a GPU: the fixture (tests/golden/reach.npz, the compiled reference's
FillRMap maps and MoveTowardsPosition moves; tests/golden/gen_reach.py) holds the hand-made cases as tests/reach_cases.py builds them,
the oracle's restatement reproduces it, the kernel's level functions compiled for the host (tests/emul/pom_reach_emul.cpp) reproduce it
in all three of the kernel's forms and for every max_dist, and equal the oracle on 10,000 random boards; move_towards on CPU tensors;
the wrapper's refusals; the header's spec."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, _ReachSpec
from pomcpp_amd.state import STATE_DTYPE, Item
from tests import reach_cases as RC
from tests import wrapper_standin as W
from tests.host_build import ROOT, header_constant, shared_lib, syntax_check
from tests.wrapper_standin import Duck

GOLDEN = os.path.join(ROOT, "tests", "golden", "reach.npz")
MAX_DISTS = (1, 2, 10, 63, 64, 120)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return {"names": list(g["names"]), "n_hand": int(g["n_hand"][0]), "states": g["states"].copy().view(STATE_DTYPE).reshape(-1),
            "map121": g["map121"], "move_to121": g["move_to121"]}


@pytest.fixture(scope="module")
def fill_rmap(oracle):
    return lambda states: RC.fill_rmap(oracle, states)


@pytest.fixture(scope="module")
def emul():
    """the kernel's level functions (pomcpp_amd/csrc/pom_reach.h) built for the host"""
    lib = C.CDLL(shared_lib("tests/emul/pom_reach_emul.cpp"))
    lib.pom_emul_reach.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]

    def run(states, max_dist=120, mask=15, dist=True, move=True, fill=0):
        """(dist, move) uint8 [n, 4, 11, 11], None for the one not asked for; rows outside the mask keep `fill`"""
        states = np.ascontiguousarray(states)
        d = np.full((states.size, 4, 11, 11), fill, dtype=np.uint8) if dist else None
        m = np.full((states.size, 4, 11, 11), fill, dtype=np.uint8) if move else None
        assert lib.pom_emul_reach(states.ctypes.data, states.size, mask, max_dist, d.ctypes.data if dist else None,
                                  m.ctypes.data if move else None) == 0
        return d, m
    return run


def test_fixture_holds_the_cases_as_they_are_built(golden):
    hand = RC.hand_made()
    assert golden["n_hand"] == len(hand) and golden["names"][:len(hand)] == [n for n, _ in hand], "the cases changed: regenerate tests/golden/reach.npz"
    for i, (name, s) in enumerate(hand):
        assert s.tobytes() == golden["states"][i:i + 1].tobytes(), name
    assert os.path.getsize(GOLDEN) < 512 * 1024
    assert len(golden["names"]) - len(hand) >= 300   # a few hundred mid-game States
    dist = golden["map121"] & 0xFFFF
    assert dist[golden["names"].index("serpentine"), 0].max() == 70   # a six-bit distance fails
    dead = golden["states"]["agents"]["dead"] != 0
    assert {int(r.sum()) for r in dead[:len(hand)]} >= {1, 2, 3} and dead[len(hand):].any() and (~dead[len(hand):]).all(axis=1).any()


def test_hand_written_rows_equal_the_fixture(golden):
    """a few rows reasoned from the reference's rules by hand"""
    dist, move = RC.expected_planes(golden["states"], golden["map121"], golden["move_to121"])
    at = golden["names"].index
    # an empty board from (0, 0): the Manhattan distance; FillRMap tries DOWN first, so every cell below row 0 is entered downwards
    d, m = dist[at("empty_0_0"), 0], move[at("empty_0_0"), 0]
    yy, xx = np.mgrid[0:11, 0:11]
    assert np.array_equal(d, yy + xx)
    assert np.array_equal(m, np.where(yy > 0, 2, np.where(xx > 0, 4, 0)))
    # from the centre (agent 0 again: the ninth spot): UP wins over RIGHT and LEFT above the source's row, DOWN below, and on the row
    # itself there is one way only
    m = move[at("empty_5_5"), 0]
    assert (m[:5] == 1).all() and (m[6:] == 2).all() and (m[5, 6:] == 4).all() and (m[5, :5] == 3).all() and m[5, 5] == 0
    # the corridor: agent 1's cell (4, 5) is reached by agent 0, what lies behind it is not; agent 1 reaches both sides
    d0, d1 = dist[at("agent_in_corridor"), 0], dist[at("agent_in_corridor"), 1]
    assert d0[5].tolist() == [0, 1, 2, 3, 4, 0, 0, 0, 0, 0, 0] and d0.sum() == 10
    assert d1[5].tolist() == [4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6]
    # the four blockers stop their arms at one step; the source stands on its own bomb and starts like any other
    d = dist[at("blockers"), 0]
    assert d.sum() == 4 and d[5, 4] == d[5, 6] == d[4, 5] == d[6, 5] == 1
    # power-ups are walked through to the arms' ends; the flame that hides one blocks
    d = dist[at("walkables"), 3]
    assert d[5].tolist() == [5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5] and d[:, 5].tolist() == [5, 4, 3, 2, 1, 0, 1, 0, 0, 0, 0]
    # the islands beside the board's edges stay unreached
    for name, x in (("leak_plus_1", 0), ("leak_minus_1", 10)):
        d = dist[at(name), 2]
        assert (d[1::2, x] == 0).all() and (d[1::2, 10 - x] != 0).all() and (d[0::2, x] == 0).all(), name
    # dead agents' rows are zero whatever the reference's search from their last cell found
    i = at("dead_03")
    assert not dist[i, 0].any() and not move[i, 3].any() and dist[i, 1].any() and (golden["map121"][i, 0] != 0).any()


def test_oracle_reproduces_the_fixture(golden, fill_rmap):
    m, mt = fill_rmap(golden["states"])
    assert np.array_equal(m, golden["map121"])
    assert np.array_equal(mt, golden["move_to121"])


@pytest.mark.parametrize("max_dist", MAX_DISTS)
def test_host_compiled_level_functions_reproduce_the_fixture(golden, emul, max_dist):
    """the labelled flood with both outputs, the labelled flood for `move` alone, the one-front flood for `dist` alone"""
    want_d, want_m = RC.expected_planes(golden["states"], golden["map121"], golden["move_to121"], max_dist)
    d, m = emul(golden["states"], max_dist)
    assert np.array_equal(d, want_d), np.argwhere(d != want_d)[:5]
    assert np.array_equal(m, want_m), np.argwhere(m != want_m)[:5]
    assert np.array_equal(emul(golden["states"], max_dist, move=False)[0], want_d)
    assert np.array_equal(emul(golden["states"], max_dist, dist=False)[1], want_m)
    if max_dist == 120:   # rows outside the mask are not written
        d, m = emul(golden["states"][:40], mask=0b0101, fill=0xAA)
        assert (d[:, [1, 3]] == 0xAA).all() and (m[:, [1, 3]] == 0xAA).all()
        assert np.array_equal(d[:, [0, 2]], want_d[:40, [0, 2]]) and np.array_equal(m[:, [0, 2]], want_m[:40, [0, 2]])


def random_boards(oracle, n, seed):
    """n boards of the device generator's distribution (include/pom_boardgen.h) with the four agents moved to random cells, a tenth
    of them dead and off the board"""
    rng = np.random.default_rng(seed)
    s = oracle.boardgen(seed, np.arange(n), np.zeros(n))
    cells = s["board"].reshape(n, 121)
    assert np.shares_memory(cells, s)
    cells[cells >= Item.AGENT0] = Item.PASSAGE
    spots = rng.permuted(np.tile(np.arange(121), (n, 1)), axis=1)[:, :4]
    dead = rng.random((n, 4)) < 0.1
    for a in range(4):
        s["agents"]["x"][:, a], s["agents"]["y"][:, a] = spots[:, a] % 11, spots[:, a] // 11
        live = ~dead[:, a]
        cells[np.nonzero(live)[0], spots[live, a]] = Item.AGENT0 + a
    s["agents"]["dead"] = dead
    s["aliveAgents"] = 4 - dead.sum(axis=1)
    return s


def test_host_compiled_level_functions_equal_the_oracle_on_random_boards(oracle, fill_rmap, emul):
    s = random_boards(oracle, 10000, 20261020)
    want_d, want_m = RC.expected_planes(s, *fill_rmap(s))
    assert want_d.max() >= 25 and (want_d != 0).sum(axis=(2, 3)).max() >= 60   # long paths and wide maps are among them
    d, m = emul(s)
    bad = np.nonzero((d != want_d).any(axis=(1, 2, 3)) | (m != want_m).any(axis=(1, 2, 3)))[0]
    assert bad.size == 0, (bad.size, bad[:5])
    assert np.array_equal(emul(s, move=False)[0], want_d) and np.array_equal(emul(s, dist=False)[1], want_m)
    for max_dist in (1, 7):
        wd, wm = RC.expected_planes(s[:2000], *fill_rmap(s[:2000]), max_dist)
        d, m = emul(s[:2000], max_dist)
        assert np.array_equal(d, wd) and np.array_equal(m, wm), max_dist


# ---- move_towards: pure torch ---------------------------------------------------------------------------------------------------
def _nearest(dist, move, targets):
    """move_towards, cell by cell"""
    out = np.zeros(dist.shape[:2], dtype=np.int32)
    for e in range(dist.shape[0]):
        for a in range(4):
            d, t = dist[e, a].reshape(121).astype(int), targets[e, a].reshape(121)
            cand = [(d[c], c) for c in range(121) if t[c] and d[c] != 0]
            if cand:
                out[e, a] = move[e, a].reshape(121)[min(cand)[1]]
    return out


def test_move_towards_on_fixture_planes(golden):
    import torch
    dist, move = RC.expected_planes(golden["states"], golden["map121"], golden["move_to121"])
    reach = {"dist": torch.from_numpy(dist), "move": torch.from_numpy(move)}
    at = golden["names"].index
    targets = np.zeros(dist.shape, dtype=bool)
    c, b, dd = at("empty_5_5"), at("blockers"), at("dead_2")
    targets[c, 0, 3, 5] = targets[c, 0, 5, 9] = True   # nearest: (5, 3) at 2 steps before (9, 5) at 4: UP
    targets[at("empty_0_0"), 0, 5, 6] = targets[at("empty_0_0"), 0, 6, 5] = True   # a tie at 11 steps: cell 61 before cell 71 — both DOWN first
    targets[at("empty_10_5"), 2, 5, 9] = targets[at("empty_10_5"), 2, 4, 10] = True   # a tie at 1 step: (10, 4) = cell 54 before (9, 5) = cell 64: UP, not LEFT
    targets[b, 0, 5, 8:] = targets[b, 0, :3, 5] = True   # behind the bomb and behind the wood: not reached
    targets[dd, 2] = True   # a dead agent reaches nothing
    targets[dd, 0, 1, 1] = True   # the source itself is no target (dist 0)
    got = pa.move_towards(reach, torch.from_numpy(targets))
    assert got.dtype == torch.int32 and tuple(got.shape) == dist.shape[:2]
    got = got.numpy()
    assert got[c, 0] == 1 and got[at("empty_0_0"), 0] == 2 and got[at("empty_10_5"), 2] == 1
    assert got[b, 0] == 0 and not got[dd].any()
    assert got.sum() == 1 + 2 + 1
    # and any targets at all, against the cell-by-cell form
    rng = np.random.default_rng(3)
    for p in (0.02, 0.3):
        targets = rng.random(dist.shape) < p
        got = pa.move_towards(reach, torch.from_numpy(targets)).numpy()
        assert np.array_equal(got, _nearest(dist, move, targets)), p
    for bad in (torch.from_numpy(targets[:, :3]), torch.from_numpy(targets.astype(np.uint8))):
        with pytest.raises(ValueError, match="targets"):
            pa.move_towards(reach, bad)


# ---- the wrapper: refusals before any library call, in the style of tests/test_wrapper_args_host.py --------------------------------
N, U8, I8 = W.N, W.U8, W.I8


def test_wrapper_refuses_bad_arguments_before_any_library_call(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = W.handle(BatchEnvironment)
    shape = (N, 4, 11, 11)
    rows = [(dict(agents=[]), "agents"), (dict(agents=[4]), "agents"), (dict(agents=16), "agents"), (dict(agents=-1), "agents"),
            (dict(agents=0), "agents"), (dict(max_dist=0), "max_dist"), (dict(max_dist=121), "max_dist"),
            (dict(dist=False, move=False), "move")]
    for name in ("dist", "move"):
        for t in (Duck(shape, I8), Duck(shape, "torch.float32"), Duck(shape + (1,), U8), Duck((N, 4, 11, 12), U8), Duck((N + 1, 4, 11, 11), U8),
                  Duck((N, 4, 121), U8), Duck(shape, U8, contiguous=False), Duck(shape, U8, device="cpu"), 0x1000):
            rows.append((dict(out={name: t}), f"out[{name!r}]"))
    for kw, named in rows:
        with pytest.raises(ValueError) as e:
            env.reach(**kw)
        assert named in str(e.value), (kw, str(e.value))
        assert not env._lib.calls, (kw, env._lib.calls)
    assert len(rows) == 8 + 18


def test_wrapper_builds_the_spec(monkeypatch):
    torch = W.standin_torch()
    monkeypatch.setitem(sys.modules, "torch", torch)
    env = W.handle(BatchEnvironment)

    def spec_of(**kw):
        torch.events.clear()
        res = env.reach(**kw)
        (entry, args), = env._lib.calls
        env._lib.calls.clear()
        assert entry == "pom_batch_reach" and isinstance(args[1]._obj, _ReachSpec)
        s = args[1]._obj
        assert s.struct_size == C.sizeof(_ReachSpec) == 40 and s.reserved_ == 0 and s.reserved2_ == 0
        return res, s, [(ev[1].address, ev[2]) for ev in torch.events if ev[0] == "fill_"]
    res, s, fills = spec_of()
    assert (s.agent_mask, s.max_dist, s.dist_dev, s.move_dev) == (15, 120, res["dist"].address, res["move"].address) and not fills
    assert res["dist"].shape == res["move"].shape == (N, 4, 11, 11) and res["dist"].dtype == res["move"].dtype == U8
    # some agents: a tensor the call allocates is zeroed first, a caller's is left alone
    mine = Duck((N, 4, 11, 11), U8)
    res, s, fills = spec_of(agents=[0, 2], max_dist=9, out={"dist": mine})
    assert (s.agent_mask, s.max_dist, s.dist_dev, s.move_dev) == (5, 9, mine.address, res["move"].address)
    assert res["dist"] is mine and fills == [(res["move"].address, 0)]
    res, s, _ = spec_of(agents=8, move=False)
    assert (s.agent_mask, s.dist_dev, s.move_dev) == (8, res["dist"].address, None) and set(res) == {"dist"}
    res, s, _ = spec_of(dist=False)
    assert (s.dist_dev, s.move_dev) == (None, res["move"].address) and set(res) == {"move"}


# ---- the header -----------------------------------------------------------------------------------------------------------------
SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomReachSpec) == POM_REACH_SPEC_SIZE ? 1 : -1];
typedef char offsets[offsetof(PomReachSpec, agent_mask) == 4 && offsetof(PomReachSpec, max_dist) == 8 && offsetof(PomReachSpec, reserved_) == 12 &&
                     offsetof(PomReachSpec, dist_dev) == 16 && offsetof(PomReachSpec, move_dev) == 24 && offsetof(PomReachSpec, reserved2_) == 32 ? 1 : -1];
int use(PomBatch* h)
{
    PomReachSpec s = {sizeof(PomReachSpec), 15, POM_REACH_MAX_DIST, 0, 0, 0, 0};
    return pom_batch_reach(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert header_constant("POM_REACH_SPEC_SIZE") == 40
    assert header_constant("POM_REACH_MAX_DIST") == 120 == pa.batch.REACH_MAX_DIST
