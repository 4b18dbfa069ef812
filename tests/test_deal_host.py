"""pom_batch_deal (include/pom_batch.h PomDealSpec) without a GPU: what every dealt board must have, on the checker's boards
(tests/deal_oracle.py) of the standard layout and of three curricula; clause 5 is unbiased; the kernel's rule functions compiled for the
host (tests/emul/pom_deal_emul.cpp) equal the checker byte for byte; dealt States are playable by the reference's rules; the library's and
the wrapper's refusals; the header's struct; the rule functions under the host sanitizers, as a stand-alone program."""
import ctypes as C
import subprocess
import sys
from collections import deque
from types import SimpleNamespace

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.batch import BatchEnvironment, _BoardLayout, _DealSpec
from pomcpp_amd.state import STATE_DTYPE, Item
from tests import deal_oracle as DO
from tests import host_build
from tests import wrapper_standin as W
from tests.wrapper_standin import Duck

SEED = 20261020
N_STANDARD = 2000
# (layout, boards): the standard one; no rigid wall and only the lanes' woods; every wood hides an item and nothing is rejected; crowded, without
# lanes — an attempt is accepted about one time in three, so that some boards run out of attempts
CURRICULA = [((0, 12, 0, 4, 0), 600), ((20, 36, 36, 121, 0), 600), ((56, 24, 10, 4, DO.NO_LANES), 2000)]


@pytest.fixture(scope="module")
def emul():
    """the kernel's rule functions (pomcpp_amd/csrc/pom_deal.h) built for the host: deal(...) as DO.deal_many, refused(states)"""
    lib = C.CDLL(host_build.shared_lib("tests/emul/pom_deal_emul.cpp"))
    lib.pom_emul_deal.argtypes = [C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.pom_emul_deal_refused.argtypes = [C.c_int, C.c_void_p]
    lib.pom_emul_deal_layout_bad.argtypes, lib.pom_emul_deal_layout_bad.restype = [C.c_void_p], C.c_char_p

    def deal(seed, envs, games, layout=DO.STANDARD, env_offset=0):
        envs = np.ascontiguousarray(np.asarray(envs) + env_offset, dtype=np.int64)
        games, lay = np.ascontiguousarray(games, dtype=np.int32), np.array(layout, dtype=np.int32)
        states, words = np.zeros(len(envs), dtype=STATE_DTYPE), np.zeros(len(envs), dtype=np.uint32)
        assert lib.pom_emul_deal(len(envs), seed & (2 ** 64 - 1), envs.ctypes.data, games.ctypes.data, lay.ctypes.data, states.ctypes.data, words.ctypes.data) == 0
        return states, words

    def refused(states):
        states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        return lib.pom_emul_deal_refused(len(states), states.ctypes.data)

    def layout_bad(layout):
        return lib.pom_emul_deal_layout_bad(np.array(layout, dtype=np.int32).ctypes.data)
    return SimpleNamespace(deal=deal, refused=refused, layout_bad=layout_bad)


@pytest.fixture(scope="module")
def boards():
    """{layout: (states, words)} of the checker: env j, game 0, for the standard layout and the curricula.  Computed once, shared, never changed."""
    out = {}
    for layout, n in [(DO.STANDARD, N_STANDARD)] + CURRICULA:
        states, words = DO.deal_many(SEED, np.arange(n), np.zeros(n, dtype=np.int64), layout)
        states.setflags(write=False)
        words.setflags(write=False)
        out[layout] = states, words
    return out


def _same(a, b):
    """two State arrays byte for byte; else the first field that differs"""
    if a.tobytes() == b.tobytes():
        return True
    for j in range(len(a)):
        for f in STATE_DTYPE.names:
            if not np.array_equal(a[j][f], b[j][f]):
                raise AssertionError(f"board {j}, {f}:\n{a[j][f]}\n{b[j][f]}")
    return False


# ---- what every dealt board has -----------------------------------------------------------------------------------------------------
def bad_by_search(board):
    """an independent breadth-first search: the passage cells no walk from (1,1) over cells that are not rigid reaches"""
    seen = np.zeros((11, 11), dtype=bool)
    seen[1, 1] = True
    queue = deque([(1, 1)])
    while queue:
        y, x = queue.popleft()
        for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
            if 0 <= ny < 11 and 0 <= nx < 11 and not seen[ny, nx] and board[ny, nx] != Item.RIGID:
                seen[ny, nx] = True
                queue.append((ny, nx))
    return int(((board == Item.PASSAGE) & ~seen).sum())


def check_invariants(states, words, layout):
    num_rigid, num_wood, num_items, max_bad, flags = layout
    board = states["board"]
    rigid, wood, flag = board == Item.RIGID, (board >> 8) == 2, board & 0xFF
    # mirror symmetry: transposing the board leaves rigid and wood where they were
    assert np.array_equal(rigid, rigid.transpose(0, 2, 1)) and np.array_equal(wood, wood.transpose(0, 2, 1))
    # the counts, and no flag but 1..3 on the woods that have one
    assert (rigid.sum((1, 2)) == num_rigid).all() and (wood.sum((1, 2)) == num_wood).all()
    assert ((wood & (flag != 0)).sum((1, 2)) == num_items).all() and (flag[wood] <= 3).all()
    assert np.isin(board[~wood & ~rigid], [Item.PASSAGE, Item.AGENT0, Item.AGENT1, Item.AGENT2, Item.AGENT3]).all()
    # clause 1 and clause 2, cell by cell ([y, x])
    for a, (x, y) in enumerate(((1, 1), (9, 1), (9, 9), (1, 9))):
        assert (board[:, y, x] == Item.AGENT0 + a).all()
        assert (states["agents"]["x"][:, a] == x).all() and (states["agents"]["y"][:, a] == y).all()
    assert ((board >= Item.AGENT0).sum((1, 2)) == 4).all()
    for line in (1, 9):
        for pos in (2, 3, 7, 8):
            assert (board[:, line, pos] == Item.PASSAGE).all() and (board[:, pos, line] == Item.PASSAGE).all()
        for pos in (4, 5, 6):
            lane = wood if not flags & DO.NO_LANES else board == Item.PASSAGE
            assert lane[:, line, pos].all() and lane[:, pos, line].all()
    for d in (0, 2, 3, 4, 5, 6, 7, 8, 10):
        assert (board[:, d, d] == Item.PASSAGE).all()
    # clause 8
    assert (states["timeStep"] == 0).all() and (states["aliveAgents"] == 4).all() and (states["bombs_count"] == 0).all() and (states["flames_count"] == 0).all()
    assert (states["agents"]["maxBombCount"] == 1).all() and (states["agents"]["bombStrength"] == 1).all() and not states["agents"]["dead"].any()
    # the word: dealt, `bad` as an independent search counts it, within the bound unless the fallback was taken
    bad, fallback, attempts = (words >> DO.BAD_SHIFT) & 0xFF, (words & DO.FALLBACK) != 0, ((words >> DO.ATTEMPTS_SHIFT) & 0xFF) + 1
    assert (words & DO.DEALT != 0).all() and (words >> 24 == 0).all() and (words & 0xFC == 0).all()
    assert [bad_by_search(b) for b in board] == bad.tolist()
    assert (bad[~fallback] <= max_bad).all() and (bad[fallback] > max_bad).all() and (attempts[fallback] == 16).all() and (attempts <= 16).all()
    return fallback, attempts


def test_standard_boards_have_what_a_pommerman_board_has(boards):
    states, words = boards[DO.STANDARD]
    fallback, attempts = check_invariants(states, words, DO.STANDARD)
    assert not fallback.any()   # the rule gives 4e-12 a board; the draws are fixed, so this run decides it once and for all
    print(f"standard layout: {attempts.mean():.3f} attempts a board, acceptance {len(attempts) / attempts.sum():.3f}")
    assert 0.7 < len(attempts) / attempts.sum() < 0.9   # about 0.8, measured with another generator
    # boards differ from env to env, and what a wood hides too
    assert len({s["board"].tobytes() for s in states[:200]}) == 200


@pytest.mark.parametrize("layout,n", CURRICULA, ids=lambda v: str(v))
def test_curricula_keep_the_invariants(boards, layout, n):
    states, words = boards[layout]
    assert len(states) == n
    fallback, attempts = check_invariants(states, words, layout)
    print(f"{layout}: {attempts.mean():.3f} attempts a board, {int(fallback.sum())} fallbacks of {n}")
    if layout[4] & DO.NO_LANES:
        assert fallback.any()   # what the flag is for
    else:
        assert not fallback.any() and (attempts == 1).all()   # nothing walls a passage off with so few rigid cells, or nothing is rejected


def test_clause_5_is_unbiased():
    """Over the first attempts of 4,000 standard boards every pair is rigid in a share within 5 binomial standard deviations of 18/40, and
    wood within 5 of 12/40 (sequential sampling: every assignment with the counts is equally likely, so every pair has the same share)."""
    n = 4000
    kinds = np.array([DO.attempt(DO.board_key(SEED, e, 0), 0, DO.STANDARD)[1] for e in range(n)])
    assert kinds.shape == (n, 40)
    for kind, p in (("rigid", 18 / 40), ("wood", 12 / 40)):
        share, sd = (kinds == kind).mean(0), (p * (1 - p) / n) ** 0.5
        assert ((kinds == kind).sum(1) == round(40 * p)).all()
        print(f"{kind}: shares {share.min():.4f} .. {share.max():.4f}, wanted {p:.3f} +- {5 * sd:.4f}")
        assert (abs(share - p) <= 5 * sd).all(), (kind, share)


def test_the_checker_refuses_what_the_rule_refuses(emul):
    good = [DO.STANDARD, (0, 12, 0, 0, 0), (80, 0, 0, 121, DO.NO_LANES), (0, 80, 80, 4, DO.NO_LANES), (56, 36, 36, 4, 0), (0, 0, 0, 0, DO.NO_LANES)]
    bad = [(35, 36, 20, 4, 0), (36, 35, 20, 4, 0), (-2, 36, 20, 4, 0), (36, 10, 4, 4, 0), (36, -2, 0, 4, DO.NO_LANES), (58, 36, 20, 4, 0),
           (82, 0, 0, 4, DO.NO_LANES), (36, 36, 37, 4, 0), (36, 36, -1, 4, 0), (36, 36, 20, -1, 0), (36, 36, 20, 122, 0), (36, 36, 20, 4, 2),
           (0, 94, 0, 4, 0), (2 ** 31 - 2, 36, 20, 4, 0)]
    for layout in good:
        assert DO.layout_ok(layout) and emul.layout_bad(layout) is None, layout
    for layout in bad:
        assert not DO.layout_ok(layout) and emul.layout_bad(layout).startswith(b"layout."), layout


# ---- the kernel's rule functions, built for the host ----------------------------------------------------------------------------------
def test_host_build_equals_the_checker(emul, boards):
    for layout, (states, words) in boards.items():   # those same boards
        n = len(states) if layout == DO.STANDARD else 200
        mine, my_words = emul.deal(SEED, np.arange(n), np.zeros(n), layout)
        assert np.array_equal(my_words, words[:n]), layout
        assert _same(mine, states[:n])
        assert emul.refused(mine) == 0
    for layout in [DO.STANDARD] + [c[0] for c in CURRICULA]:   # other games and another part of a sharded job
        for offset in (0, 10 ** 6):
            envs, games = np.repeat(np.arange(12), 4), np.tile([0, 1, 7, 2 ** 31 - 1], 12)
            want, want_words = DO.deal_many(SEED + 1, envs, games, layout, offset)
            mine, my_words = emul.deal(SEED + 1, envs, games, layout, offset)
            assert np.array_equal(my_words, want_words) and _same(mine, want)
            # every (env, game) its own board — but where the layout leaves nothing to draw
            assert len({s.tobytes() for s in want}) == (1 if layout[:3] == (0, 12, 0) else len(want))
    # the key is (seed, env_offset + env, game): the same board under two names
    a, aw = emul.deal(5, [3], [2], DO.STANDARD, 10 ** 6)
    b, bw = DO.deal(5, 10 ** 6 + 3, 2)
    assert a.tobytes() == b.tobytes() and aw[0] == bw
    assert DO.next_game(np.array([0, 6, 2 ** 31 - 1])).tolist() == [1, 7, -2 ** 31]


def test_dealt_states_are_playable(oracle, emul, boards):
    """64 dealt States under SimpleAgent x4 for 60 ticks: Oracle.run_simple's loop, played tick by tick so that every tick's POM_UB_*
    flags are seen (run_simple drops them) and equal to run_simple's result at the end; and the States survive pack -> unpack bit for bit."""
    start = np.ascontiguousarray(boards[DO.STANDARD][0][:64])
    assert emul.refused(start) == 0
    n, ticks, seed = len(start), 60, 9
    s, mems = start.copy(), np.zeros((n, 4, 16), dtype=np.int32)
    for t in range(ticks):
        over = s["aliveAgents"] <= 1
        s[over], mems[over] = start[over], 0
        flags = oracle.step_batch(s, oracle.simple_policy(s, mems, seed, 0, t))
        assert not flags.any(), (t, np.flatnonzero(flags), flags[flags != 0])
        s["timeStep"] += 1
    ref, ref_mems = start.copy(), np.zeros((n, 4, 16), dtype=np.int32)
    oracle.run_simple(ref, start, ref_mems, ticks, seed, 0, 0, 0)
    assert ref.tobytes() == s.tobytes() and np.array_equal(ref_mems, mems)
    # the games went somewhere: wood burnt, power-ups picked up, agents died
    assert ((s["board"] >> 8) == 2).sum() < ((start["board"] >> 8) == 2).sum() and (s["agents"]["bombStrength"] > 1).any() and (s["aliveAgents"] < 4).any()


# ---- the library's refusals that need no device: pom_deal.hip checks the spec before the handle ----------------------------------------
def _spec_of(**kw):
    fields = dict(mode=0, which=0, reserved_=0, first=0, count=4, seed=1, layout=DO.STANDARD, reserved2_=0, games_dev=0x1000, which_dev=None,
                  result_dev=0x4000, stream=None)
    fields.update(kw)
    size = fields.pop("struct_size", C.sizeof(_DealSpec))
    fields["layout"] = _BoardLayout(*fields["layout"])
    return _DealSpec(size, *[fields[f] for f, _ in _DealSpec._fields_[1:]])


def test_library_refuses_a_bad_spec_by_name(hip_lib):
    lib = hip_lib

    def refusal(**kw):
        spec = _spec_of(**kw)
        assert lib.pom_batch_create(None, 0, None) == 1   # another call's text
        assert lib.pom_batch_deal(None, C.byref(spec)) == 1   # POM_E_ARG
        text = lib.pom_last_error().decode()
        assert text.startswith("pom_batch_deal: "), text
        return text
    assert "handle is NULL" in refusal()   # a good spec gets as far as the handle
    assert "handle is NULL" in refusal(count=0, games_dev=None, result_dev=None)
    assert "handle is NULL" in refusal(mode=1, which=1, which_dev=0x2000, layout=(56, 24, 10, 4, 1))
    assert "handle is NULL" in refusal(which=2) and "handle is NULL" in refusal(which=3)
    for kw, named in ((dict(struct_size=88), "struct_size"), (dict(struct_size=104), "struct_size"), (dict(reserved_=1), "reserved_"),
                      (dict(reserved2_=1), "reserved2_"), (dict(mode=2), "mode"), (dict(mode=-1), "mode"), (dict(which=4), "which"), (dict(which=-1), "which"),
                      (dict(layout=(35, 36, 20, 4, 0)), "num_rigid"), (dict(layout=(-2, 36, 20, 4, 0)), "num_rigid"), (dict(layout=(36, 37, 20, 4, 0)), "num_wood"),
                      (dict(layout=(36, 10, 4, 4, 0)), "lane woods"), (dict(layout=(58, 36, 20, 4, 0)), "40 pairs"), (dict(layout=(82, 0, 0, 4, 1)), "40 pairs"),
                      (dict(layout=(36, 36, 37, 4, 0)), "num_items"), (dict(layout=(36, 36, -1, 4, 0)), "num_items"),
                      (dict(layout=(36, 36, 20, 122, 0)), "max_inaccessible"), (dict(layout=(36, 36, 20, -1, 0)), "max_inaccessible"),
                      (dict(layout=(36, 36, 20, 4, 2)), "flags"), (dict(count=-1), "count"), (dict(games_dev=None), "games_dev is NULL"),
                      (dict(which=1), "which_dev is NULL"), (dict(games_dev=0x1002), "4-byte"), (dict(which=1, which_dev=0x2001), "4-byte"),
                      (dict(result_dev=0x4002), "4-byte")):
        assert named in refusal(**kw), kw
    assert lib.pom_batch_deal(None, None) == 1 and lib.pom_last_error().decode().startswith("pom_batch_deal: the spec is NULL")


# ---- the wrapper: refusals before any library call, and the spec it builds ---------------------------------------------------------
N, I32, U8 = W.N, W.I32, W.U8


def test_wrapper_refuses_bad_arguments_before_any_library_call(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    env = W.handle(BatchEnvironment)
    games = Duck((N,), I32)
    rows = [(dict(mode="begin"), "mode"), (dict(which="some"), "which"), (dict(which=Duck((N - 1,), I32)), "which"), (dict(which=Duck((N,), U8)), "which"),
            (dict(which=None), "which"), (dict(first=-1), "outside the batch"), (dict(first=N + 1), "outside the batch"), (dict(first=4, count=N - 3), "outside the batch"),
            (dict(count=-1), "outside the batch"), (dict(games=Duck((N + 1,), I32)), "games"), (dict(games=Duck((N,), "torch.int64")), "games"),
            (dict(games=None), "games"), (dict(games=np.zeros(N, dtype=np.int32)), "games"), (dict(games=Duck((N,), I32, contiguous=False)), "games"),
            (dict(games=Duck((N,), I32, device="cpu")), "games"), (dict(layout=(36, 36, 20, 4, 0)), "layout"), (dict(out=Duck((N - 1,), I32)), "out"),
            (dict(out=Duck((N,), U8)), "out")]
    for kw, named in rows:
        args = dict(games=games)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            env.deal(**args)
        assert named in str(e.value), (kw, str(e.value))
        assert not env._lib.calls, (kw, env._lib.calls)
    for kw, named in ((dict(num_rigid=35), "num_rigid"), (dict(num_wood=10), "num_wood"), (dict(num_rigid=58), "40"), (dict(num_items=37), "num_items"),
                      (dict(max_inaccessible=122), "max_inaccessible"), (dict(num_rigid=82, num_wood=0, num_items=0, no_lanes=True), "40")):
        with pytest.raises(ValueError) as e:
            pa.BoardLayout(**kw)
        assert named in str(e.value), (kw, str(e.value))
    assert pa.BoardLayout().as_tuple() == DO.STANDARD and pa.BoardLayout(56, 24, 10, 4, no_lanes=True).as_tuple() == (56, 24, 10, 4, 1)


def test_wrapper_builds_the_spec(monkeypatch):
    monkeypatch.setitem(sys.modules, "torch", W.standin_torch())
    events = []
    env = W.handle(BatchEnvironment, events=events)

    def spec_of(**kw):
        out = env.deal(**kw)
        (entry, args), = env._lib.calls
        env._lib.calls.clear()
        assert entry == "pom_batch_deal" and isinstance(args[1]._obj, _DealSpec)
        s = args[1]._obj
        assert s.struct_size == C.sizeof(_DealSpec) == 96 and s.reserved_ == 0 and s.reserved2_ == 0
        return s, out

    def layout_of(s):
        return tuple(getattr(s.layout, f) for f, _ in _BoardLayout._fields_)
    games = Duck((N,), I32)
    s, out = spec_of(games=games)
    assert (s.mode, s.which, s.first, s.count, s.seed, layout_of(s)) == (0, 0, 0, N, 0, DO.STANDARD) and len(events) == 1   # (ordered with torch's stream)
    assert (s.games_dev, s.which_dev, s.result_dev, s.stream) == (games.address, None, None, None) and out is None
    mask, words = Duck((N,), I32), Duck((N,), I32)
    s, out = spec_of(games=games, seed=-1, mode="next", which=mask, first=3, count=11, layout=pa.BoardLayout(56, 24, 10, 4, no_lanes=True), out=words,
                     stream=SimpleNamespace(cuda_stream=0x77))
    assert out is words and len(events) == 1   # a caller's stream orders the call: nothing is waited for
    assert (s.mode, s.which, s.first, s.count, s.seed, layout_of(s), s.stream) == (1, 1, 3, 11, 2 ** 64 - 1, (56, 24, 10, 4, 1), 0x77)
    assert (s.games_dev, s.which_dev, s.result_dev) == (games.address, mask.address, words.address)
    for which, code in (("all", 0), ("restarted", 2), ("done", 3)):
        s, _ = spec_of(games=games, which=which, first=5, stream=0x99)
        assert (s.which, s.first, s.count, s.which_dev, s.stream) == (code, 5, N - 5, None, 0x99)
    s, _ = spec_of(games=games, first=N)   # an empty range: no address is passed
    assert s.count == 0 and s.games_dev is None


def test_decode_deal_names_the_fields():
    w = np.array([0, 1, 1 | (2 << 8) | (3 << 16), 1 | 2 | (15 << 8) | (121 << 16)], dtype=np.uint32)
    d = pa.decode_deal(w)
    assert d["dealt"].tolist() == [False, True, True, True] and d["fallback"].tolist() == [False, False, False, True]
    assert d["attempts"].tolist() == [0, 1, 3, 16] and d["bad"].tolist() == [0, 0, 3, 121]
    d32 = pa.decode_deal(w.view(np.int32))
    assert all(np.array_equal(d[k], d32[k]) for k in d)
    assert (pa.batch.DEAL_DEALT, pa.batch.DEAL_FALLBACK, pa.batch.DEAL_ATTEMPTS_SHIFT, pa.batch.DEAL_BAD_SHIFT) == (DO.DEALT, DO.FALLBACK, DO.ATTEMPTS_SHIFT, DO.BAD_SHIFT)


# ---- the header -----------------------------------------------------------------------------------------------------------------
SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomDealSpec) == POM_DEAL_SPEC_SIZE && sizeof(PomDealSpec) == 96 && sizeof(PomBoardLayout) == 20 ? 1 : -1];
typedef char offsets[offsetof(PomDealSpec, mode) == 4 && offsetof(PomDealSpec, which) == 8 && offsetof(PomDealSpec, reserved_) == 12 &&
                     offsetof(PomDealSpec, first) == 16 && offsetof(PomDealSpec, count) == 24 && offsetof(PomDealSpec, seed) == 32 &&
                     offsetof(PomDealSpec, layout) == 40 && offsetof(PomDealSpec, reserved2_) == 60 && offsetof(PomDealSpec, games_dev) == 64 &&
                     offsetof(PomDealSpec, which_dev) == 72 && offsetof(PomDealSpec, result_dev) == 80 && offsetof(PomDealSpec, stream) == 88 &&
                     offsetof(PomBoardLayout, num_wood) == 4 && offsetof(PomBoardLayout, num_items) == 8 &&
                     offsetof(PomBoardLayout, max_inaccessible) == 12 && offsetof(PomBoardLayout, flags) == 16 ? 1 : -1];
typedef char words[POM_DEAL_START == 0 && POM_DEAL_NEXT == 1 && POM_DEAL_ALL == 0 && POM_DEAL_MASK == 1 && POM_DEAL_RESTARTED == 2 && POM_DEAL_DONE == 3 &&
                   POM_DEAL_DEALT == 1 && POM_DEAL_FALLBACK == 2 && POM_LAYOUT_NO_LANES == 1 ? 1 : -1];
int use(PomBatch* h, int32_t* games)
{
    PomDealSpec s = {sizeof(PomDealSpec), POM_DEAL_NEXT, POM_DEAL_RESTARTED, 0, 0, 16, 1, {36, 36, 20, 4, 0}, 0, games, 0, 0, 0};
    return pom_batch_deal(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    host_build.syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert C.sizeof(_DealSpec) == 96 and C.sizeof(_BoardLayout) == 20
    assert [(f, getattr(_DealSpec, f).offset) for f in ("layout", "reserved2_", "games_dev", "stream")] == [("layout", 40), ("reserved2_", 60), ("games_dev", 64), ("stream", 88)]


# ---- the rule functions under the host sanitizers: a stand-alone program, run as a child process --------------------------------------
def test_rule_functions_under_the_sanitizers():
    exe = host_build.program("tests/emul/pom_deal_emul.cpp", name="pom_deal_emul_asan", extra=["-DPOM_DEAL_EMUL_MAIN"], sanitize=True)
    r = subprocess.run([exe, "20000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "20000 boards of 4 layouts ok" in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr
