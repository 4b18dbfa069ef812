"""pom_batch_imagine (include/pom_batch.h PomImagineSpec) without a GPU: the checker (tests/imagine_oracle.py) builds what was reasoned
by hand on the hand-made cases (tests/imagine_cases.py); the kernel's rule functions compiled for the host (tests/emul/
pom_imagine_emul.cpp) equal the checker on those cases and on the views of a batch of SimpleAgent games played by the CPU oracle; the
checker's States are playable by the reference's rules; the library's and the wrapper's refusals; the header's struct."""
import ctypes as C
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, _ImagineSpec
from pomcpp_amd.state import STATE_DTYPE, Item
from tests import imagine_cases as IC
from tests import imagine_oracle as IO
from tests import view_memory_oracle as VM
from tests import wrapper_standin as W
from tests.host_build import ROOT, shared_lib, syntax_check
from tests.view_oracle import viewer_attrs
from tests.wrapper_standin import Duck

UNKNOWN = {"sample": IO.SAMPLE, "passage": IO.PASSAGE}
CASES = IC.cases()


@pytest.fixture(scope="module")
def obs():
    spec = importlib.util.spec_from_file_location("pom_observe_oracle", os.path.join(ROOT, "oracle", "pom_observe_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def emul():
    """the kernel's rule functions (pomcpp_amd/csrc/pom_imagine.h) built for the host: imagine(...) as IO.imagine, refused(states)"""
    lib = C.CDLL(shared_lib("tests/emul/pom_imagine_emul.cpp"))
    lib.pom_emul_imagine.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.pom_emul_imagine_refused.argtypes = [C.c_int, C.c_void_p]

    def imagine(memory, attrs, view, sample=None, seed=0, unknown=IO.SAMPLE, belief=None):
        memory, attrs = np.ascontiguousarray(memory, dtype=np.uint8), np.ascontiguousarray(attrs, dtype=np.int32)
        view = np.ascontiguousarray(view, dtype=np.int32)
        sample = None if sample is None else np.ascontiguousarray(sample, dtype=np.int32)
        belief = None if belief is None else np.ascontiguousarray(belief, dtype=np.int32)
        states, words = np.zeros(len(view), dtype=STATE_DTYPE), np.zeros(len(view), dtype=np.uint32)
        assert lib.pom_emul_imagine(len(view), view.ctypes.data, None if sample is None else sample.ctypes.data, 4 * len(memory), memory.ctypes.data,
                                    attrs.ctypes.data, None if belief is None else belief.ctypes.data, seed, unknown, states.ctypes.data,
                                    words.ctypes.data) == 0
        return states, words

    def refused(states):
        states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        return lib.pom_emul_imagine_refused(len(states), states.ctypes.data)
    return SimpleNamespace(imagine=imagine, refused=refused)


def _same(a, b):
    """two State arrays byte for byte; else the first field that differs"""
    if a.tobytes() == b.tobytes():
        return True
    for j in range(len(a)):
        for f in STATE_DTYPE.names:
            if not np.array_equal(a[j][f], b[j][f]):
                raise AssertionError(f"job {j}, {f}:\n{a[j][f]}\n{b[j][f]}")
    return False


def test_the_cases_cover_every_clause():
    assert {c["name"] for c in CASES} >= {
        "wiped_viewer_alone", "bomb_under_an_agent", "21_bombs", "21_flame_pieces", "flames_L_and_cross", "dead_viewer", "dead_enemys_stale_code",
        "no_room", "garbage_byte_on_a_known_cell", "unseen_enemy_where_the_viewer_does_not_look", "unseen_enemy_all_seen",
        "clamped_bombs_and_flames", "clamped_viewer_attrs"}
    assert len(CASES) == 13


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_checker_builds_what_was_reasoned_by_hand_and_the_host_build_equals_it(emul, case):
    args = (case["memory"], case["attrs"], [case["view"]], [3], 0x5EED, UNKNOWN[case["unknown"]], case["belief"])
    states, words = IO.imagine(*args)
    case["expect"](states[0], int(words[0]))
    mine, my_words = emul.imagine(*args)
    assert np.array_equal(my_words, words), (hex(my_words[0]), hex(words[0]))
    assert _same(mine, states)
    if words[0] & IO.BUILT:
        assert emul.refused(states) == 0
    # both ways of filling the unknown, other samples, the slot (the job's place in the list) and "no job" entries beside it
    for unknown in UNKNOWN.values():
        view, sample = [-1, case["view"], 4, case["view"], case["view"]], [0, 1, 2, 1, 7]
        a, aw = IO.imagine(case["memory"], case["attrs"], view, sample, 99, unknown, case["belief"])
        b, bw = emul.imagine(case["memory"], case["attrs"], view, sample, 99, unknown, case["belief"])
        assert np.array_equal(aw, bw) and _same(a, b) and aw[0] == 0 and aw[2] == 0 and aw[1] == aw[3] and a[1] == a[3]


# ---- playable by the reference's rules ----------------------------------------------------------------------------------------------
def _flame_ids(board):
    return {(int(v) - Item.FLAMES) >> 3 for v in board.reshape(-1) if v >> 16 == 4}


def playable(oracle, state, ticks=12):
    """`ticks` of the oracle's Step under idle moves from a State the checker built without a drop flag.  No tick raises a POM_UB_* flag.
    Every flame is gone by its life and every bomb explodes at its life: after each tick no queued flame has timeLeft <= 0 and no queued
    bomb time 0 (the queues are in order, so the head is popped when it is due), and there are never more bombs than those of the start
    whose life is longer than the ticks played (a flame may set one off earlier; nobody plants).  PopFlame leaves no orphan: every flame
    cell on the board carries the origin of a queued flame.  Returns a text for the first thing wrong, or None."""
    s = np.array([state], dtype=STATE_DTYPE)
    st = s[0]
    times = [(int(b) >> 16) & 15 for b in st["bombs_queue"][:int(st["bombs_count"])]]
    if _flame_ids(st["board"]) != {int(f["x"]) + 11 * int(f["y"]) for f in st["flames_queue"][:int(st["flames_count"])]}:
        return "a flame cell without its flame, or a flame without cells, at the start"
    for tick in range(1, ticks + 1):
        if oracle.step(s, [0, 0, 0, 0]):
            return f"tick {tick}: a POM_UB flag"
        bombs = [int(st["bombs_queue"][(int(st["bombs_index"]) + k) % 20]) for k in range(int(st["bombs_count"]))]
        flames = [st["flames_queue"][(int(st["flames_index"]) + k) % 20] for k in range(int(st["flames_count"]))]
        if any(int(f["timeLeft"]) <= 0 for f in flames):
            return f"tick {tick}: a flame outlives its life"
        if not _flame_ids(st["board"]) <= {int(f["x"]) + 11 * int(f["y"]) for f in flames}:
            return f"tick {tick}: orphan flame cells"
        if any((b >> 16) & 15 == 0 for b in bombs) or len(bombs) > sum(t > tick for t in times):
            return f"tick {tick}: a bomb outlives its life, or a new one"
    return None


@pytest.mark.parametrize("case", [c for c in CASES if c["playable"]], ids=lambda c: c["name"])
def test_the_cases_states_are_playable(oracle, emul, case):
    for unknown in UNKNOWN.values():
        states, words = IO.imagine(case["memory"], case["attrs"], [case["view"]] * 4, None, 5, unknown, case["belief"])
        assert (words & 15 == IO.BUILT).all() and emul.refused(states) == 0
        for s in states:
            assert playable(oracle, s) is None


# ---- a batch played on the CPU: the shape of tests/test_gpu_imagine.py's batch ------------------------------------------------------------
N_GAMES, TICKS, SEED, BSEED = 48, 40, 20261020, 11


@pytest.fixture(scope="module")
def remembered(oracle, obs):
    """SimpleAgent x4 on N_GAMES generated boards for TICKS ticks, every agent remembering at radius 4 each tick: (memory, viewer_attrs)
    after the last tick.  Computed once, shared, never changed."""
    n = N_GAMES
    states = oracle.boardgen(BSEED, np.arange(n), np.zeros(n))
    eps, mems = np.zeros(n, dtype=np.int32), np.zeros((n, 4, 16), dtype=np.int32)
    memory, stamp = VM.new_memory(n)
    for tick in range(TICKS + 1):
        _, attrs, env2 = obs.observe(states)
        env = np.zeros((n, 4), dtype=np.int32)
        env[:, :2] = env2
        VM.remember(memory, stamp, obs.observe_codes(states), attrs, env, eps.astype(np.uint32), 4)
        va = viewer_attrs(attrs, env[:, 0])
        if tick < TICKS:
            oracle.run_simple_fresh(states, eps, mems, 1, SEED, BSEED, 0, tick, 0)
    memory.setflags(write=False)
    va.setflags(write=False)
    return memory, va


def test_host_build_equals_the_checker_on_played_games_and_the_states_are_playable(oracle, emul, remembered):
    """Every view of every env, samples 0..3: 768 jobs.  The checker's count of jobs with a drop flag on this batch is 0 of 768 —
    tests/test_gpu_imagine.py relies on at most 1 in 10 for its round trip."""
    memory, va = remembered
    view = np.repeat(np.arange(4 * N_GAMES), 4)
    sample = np.tile(np.arange(4), 4 * N_GAMES)
    states, words = IO.imagine(memory, va, view, sample, SEED, IO.SAMPLE)
    mine, my_words = emul.imagine(memory, va, view, sample, SEED, IO.SAMPLE)
    assert np.array_equal(my_words, words) and _same(mine, states)
    built = (words & IO.BUILT) != 0
    dropped = (words & (IO.DROPPED_BOMBS | IO.DROPPED_FLAMES)) != 0
    print(f"built {built.sum()} of {len(words)}, with a drop flag {dropped.sum()}, no room {(words == IO.NO_ROOM).sum()}")
    assert built.sum() >= 0.9 * len(words) and dropped.sum() * 10 <= len(words)
    assert emul.refused(states[built]) == 0
    # the batch exercises the rule: unknown cells, drawn agents, remembered agents, bombs and flames
    assert ((words >> 8) & 0xFF).max() > 60 and ((words >> 16) & 15).any() and states["bombs_count"].any() and states["flames_count"].any()
    wrong = [(j, why) for j in np.flatnonzero(built & ~dropped)[::3] for why in [playable(oracle, states[j])] if why]
    assert not wrong, wrong[:5]
    # two samples of a view show the same on every known cell — as codes: what a wood hides is drawn — but where a drawn agent stands,
    # differ somewhere, and the same (view, sample) is the same game whatever its place in the list
    known = IO.known_cells(memory.reshape(-1, 6, 121).astype(np.int64))[view].reshape(-1, 11, 11)
    codes, free = IO.board_codes(states["board"]), ~IO.drawn_cells(states, words)
    both = built[0::4] & built[1::4]
    agree = np.where(known[0::4] & free[0::4] & free[1::4], codes[0::4] == codes[1::4], True)
    assert agree[both].all() and (states["board"][0::4] != states["board"][1::4])[both].any()
    order = np.random.default_rng(1).permutation(len(view))
    again, again_words = IO.imagine(memory, va, view[order], sample[order], SEED, IO.SAMPLE)
    assert np.array_equal(again_words, words[order]) and _same(again, states[order])


# ---- the library's refusals that need no device: pom_memory.hip checks the spec before the handle -------------------------------
def test_library_refuses_a_bad_spec_by_name(hip_lib):
    lib = hip_lib

    def refusal(**kw):
        fields = dict(unknown=0, first=0, count=4, rows=8, reserved_=0, seed=1, view_dev=0x1000, sample_dev=None, memory_dev=0x2000,
                      viewer_attrs_dev=0x3000, belief_attrs_dev=None, result_dev=0x4000, stream=None)
        fields.update(kw)
        size = fields.pop("struct_size", C.sizeof(_ImagineSpec))
        spec = _ImagineSpec(size, *[fields[f] for f, _ in _ImagineSpec._fields_[1:]])
        assert lib.pom_batch_create(None, 0, None) == 1   # another call's text
        assert lib.pom_batch_imagine(None, C.byref(spec)) == 1   # POM_E_ARG
        text = lib.pom_last_error().decode()
        assert text.startswith("pom_batch_imagine: "), text
        return text
    assert "handle is NULL" in refusal()   # a good spec gets as far as the handle
    assert "handle is NULL" in refusal(count=0, view_dev=None, memory_dev=None, viewer_attrs_dev=None)
    for kw, named in ((dict(struct_size=88), "struct_size"), (dict(reserved_=1), "reserved_"), (dict(unknown=2), "unknown"), (dict(unknown=-1), "unknown"),
                      (dict(rows=0), "rows"), (dict(rows=6), "rows"), (dict(rows=-4), "rows"), (dict(count=-1), "count"),
                      (dict(view_dev=None), "view_dev is NULL"), (dict(memory_dev=None), "memory_dev is NULL"),
                      (dict(viewer_attrs_dev=None), "viewer_attrs_dev is NULL"), (dict(view_dev=0x1002), "4-byte"), (dict(sample_dev=0x1001), "4-byte"),
                      (dict(memory_dev=0x2002), "4-byte"), (dict(result_dev=0x4002), "4-byte"), (dict(viewer_attrs_dev=0x3008), "16-byte"),
                      (dict(belief_attrs_dev=0x5004), "16-byte")):
        assert named in refusal(**kw), kw
    assert lib.pom_batch_imagine(None, None) == 1 and lib.pom_last_error().decode().startswith("pom_batch_imagine: the spec is NULL")


# ---- the wrapper: refusals before any library call, and the spec it builds ---------------------------------------------------------
N, M, U8, I32 = W.N, W.M, W.U8, W.I32


def _args(**kw):
    args = dict(memory=Duck((N, 4, 6, 11, 11), U8), viewer_attrs=Duck((N, 4, 12), I32), view=Duck((M,), I32))
    args.update(kw)
    return args


def test_wrapper_refuses_bad_arguments_before_any_library_call(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = W.handle(BatchEnvironment)
    rows = [(dict(unknown="fog"), "unknown"), (dict(first=-1), "outside the batch"), (dict(first=N - M + 1), "outside the batch"),
            (dict(view=Duck((M, 1), I32)), "view"), (dict(view=Duck((M,), "torch.int64")), "view"), (dict(view=None), "view"),
            (dict(view=np.zeros(M, dtype=np.float32)), "view"), (dict(sample=Duck((M + 1,), I32)), "sample"), (dict(sample=Duck((M,), U8)), "sample"),
            (dict(memory=Duck((N, 4, 5, 11, 11), U8)), "memory"), (dict(memory=Duck((N, 4, 6, 11, 11), I32)), "memory"),
            (dict(memory=Duck((N, 4, 6, 11, 11), U8, contiguous=False)), "memory"), (dict(memory=Duck((N, 4, 6, 11, 11), U8, device="cpu")), "memory"),
            (dict(memory=None), "memory"), (dict(viewer_attrs=Duck((N, 4, 8), I32)), "viewer_attrs"), (dict(viewer_attrs=Duck((N - 1, 4, 12), I32)), "viewer_attrs"),
            (dict(viewer_attrs=None), "viewer_attrs"), (dict(belief=Duck((N, 4, 4), I32)), "belief"), (dict(belief=Duck((N, 4, 4, 3), U8)), "belief"),
            (dict(out=Duck((M + 1,), I32)), "out"), (dict(out=Duck((M,), U8)), "out")]
    for kw, named in rows:
        with pytest.raises(ValueError) as e:
            env.imagine(**_args(**kw))
        assert named in str(e.value), (kw, str(e.value))
        assert not env._lib.calls, (kw, env._lib.calls)


def test_wrapper_builds_the_spec(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    events = []
    env = W.handle(BatchEnvironment, events=events)

    def spec_of(**kw):
        out = env.imagine(**kw)
        (entry, args), = env._lib.calls
        env._lib.calls.clear()
        assert entry == "pom_batch_imagine" and isinstance(args[1]._obj, _ImagineSpec)
        s = args[1]._obj
        assert s.struct_size == C.sizeof(_ImagineSpec) == 96 and s.reserved_ == 0
        return s, out
    a = _args()
    s, out = spec_of(**a)
    assert (s.unknown, s.first, s.count, s.rows, s.seed) == (0, 0, M, 4 * N, 0) and len(events) == 1   # (ordered with torch's stream)
    assert (s.view_dev, s.sample_dev, s.memory_dev, s.viewer_attrs_dev, s.belief_attrs_dev, s.result_dev, s.stream) == \
        (a["view"].address, None, a["memory"].address, a["viewer_attrs"].address, None, out.address, None)
    assert tuple(out.shape) == (M,) and out.dtype == I32
    a = _args(memory=Duck((3, 4, 6, 11, 11), U8), viewer_attrs=Duck((3, 4, 12), I32), sample=Duck((M,), I32), belief=Duck((3, 4, 4, 3), I32),
              out=Duck((M,), I32), first=N - M, seed=-1, unknown="passage", stream=SimpleNamespace(cuda_stream=0x77))
    s, out = spec_of(**a)
    assert out is a["out"] and len(events) == 1   # a caller's stream orders the call: nothing is waited for
    assert (s.unknown, s.first, s.count, s.rows, s.seed, s.stream) == (1, N - M, M, 12, 2 ** 64 - 1, 0x77)
    assert (s.sample_dev, s.belief_attrs_dev, s.result_dev) == (a["sample"].address, a["belief"].address, out.address)
    s, out = spec_of(**_args(view=np.array([0, 5, -1], dtype=np.int64)))   # a numpy list is copied to the device
    assert s.count == 3 and s.view_dev is not None


def test_decode_imagine_names_the_fields():
    w = np.array([0, 8, 1 | (121 << 8), 1 | 2 | 4 | (7 << 8) | (0b1010 << 16)], dtype=np.uint32)
    d = pa.decode_imagine(w)
    assert d["built"].tolist() == [False, False, True, True] and d["no_room"].tolist() == [False, True, False, False]
    assert d["dropped_bombs"].tolist() == [False, False, False, True] == d["dropped_flames"].tolist()
    assert d["unknown"].tolist() == [0, 0, 121, 7] and d["drawn"][3].tolist() == [False, True, False, True] and not d["drawn"][:3].any()
    d32 = pa.decode_imagine(w.view(np.int32))
    assert all(np.array_equal(d[k], d32[k]) for k in d)


# ---- the header -----------------------------------------------------------------------------------------------------------------
SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomImagineSpec) == POM_IMAGINE_SPEC_SIZE ? 1 : -1];
typedef char offsets[offsetof(PomImagineSpec, unknown) == 4 && offsetof(PomImagineSpec, first) == 8 && offsetof(PomImagineSpec, count) == 16 &&
                     offsetof(PomImagineSpec, rows) == 24 && offsetof(PomImagineSpec, seed) == 32 && offsetof(PomImagineSpec, view_dev) == 40 &&
                     offsetof(PomImagineSpec, result_dev) == 80 && offsetof(PomImagineSpec, stream) == 88 ? 1 : -1];
int use(PomBatch* h, const int32_t* view, const uint8_t* memory, const int32_t* attrs)
{
    PomImagineSpec s = {sizeof(PomImagineSpec), POM_IMAGINE_SAMPLE, 0, 16, 64, 0, 1, view, 0, memory, attrs, 0, 0, 0};
    return pom_batch_imagine(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert (pa.batch.IMAGINE_BUILT, pa.batch.IMAGINE_DROPPED_BOMBS, pa.batch.IMAGINE_DROPPED_FLAMES, pa.batch.IMAGINE_NO_ROOM) == \
        (IO.BUILT, IO.DROPPED_BOMBS, IO.DROPPED_FLAMES, IO.NO_ROOM) == (1, 2, 4, 8)
