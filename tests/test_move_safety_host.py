"""pom_batch_move_safety (include/pom_batch.h PomMoveSafetySpec) without a GPU: the checker (tests/move_safety_oracle.py: K x
Oracle.step per candidate, R as a boolean array) equals the compiled reference's answers (tests/golden/move_safety.npz,
tests/golden/gen_move_safety.py) on every case, the hand-made cases give the rows written out by hand below, the header's spec compiles
as C and C++ at the size it states, and the kernel's two set functions, compiled for the host, equal the checker's boolean arrays."""
import ctypes as C
import os

import numpy as np
import pytest

import pomcpp_amd as pa
from pomcpp_amd.state import STATE_DTYPE
from tests import forecast_cases as FC
from tests import move_safety_cases as MC
from tests.host_build import ROOT, header_constant, shared_lib, syntax_check
from tests.move_safety_oracle import free_cells, grow, move_safety

GOLDEN = os.path.join(ROOT, "tests", "golden", "move_safety.npz")

# What agent 0 of each hand-made case of tests/move_safety_cases.py must get, (death_tick row, escape_tick row), the columns IDLE, UP,
# DOWN, LEFT, RIGHT, BOMB; reasoned from the reference's rules: UP is y - 1 and a move off the board or into a wall leaves the agent
# where it is; a bomb planted by a move goes off in tick 11 (planted with BOMB_LIFETIME + 1 and ticked in the same Step, step.cpp:54)
# and one planted with life L in tick L; its cross reaches `strength` cells; an agent in a cell that catches fire dies in that tick.
HAND = {
    # (0, 0) on an empty board: UP and LEFT leave the board, DOWN and RIGHT are steps, nothing burns — but for BOMB: it goes off under
    # the agent that stands still in tick 11.  The walker has ten ticks on an open board: R is never empty
    "open_corner": ([0, 0, 0, 0, 0, 11], [0, 0, 0, 0, 0, 0]),
    # (1, 0) and (0, 1) rigid: no move moves, R = {(0, 0)} until the bomb takes the cell in tick 11
    "closed_corner": ([0, 0, 0, 0, 0, 11], [0, 0, 0, 0, 0, 11]),
    # the walker can reach (0, 0), (1, 0), (2, 0) and the strength-2 cross from (0, 0) is exactly these: all burn in tick 11.  RIGHT is
    # a step to (1, 0) and plants nothing
    "corridor_too_short": ([0, 0, 0, 0, 0, 11], [0, 0, 0, 0, 0, 11]),
    # (3, 0) is open too and the cross ends at (2, 0)
    "corridor_long_enough": ([0, 0, 0, 0, 0, 11], [0, 0, 0, 0, 0, 0]),
    # agent on (5, 5), the cross of the bomb on (3, 5), strength 2, is (1..5, 5) and (3, 3..7) and burns in tick 3.  IDLE, LEFT
    # (to (4, 5)) and BOMB stay inside: dead in tick 3; UP, DOWN, RIGHT step out.  Every walker has two ticks to leave the row: escape 0
    "bomb_nearby": ([3, 0, 0, 3, 0, 3], [0, 0, 0, 0, 0, 0]),
    # the same cross going off in tick 1: the three candidates that stay inside are dead after tick 1 and R_1 is empty with them
    "step_out": ([1, 0, 0, 1, 0, 1], [1, 0, 0, 1, 0, 1]),
    "stay_in": ([1, 0, 0, 1, 0, 1], [1, 0, 0, 1, 0, 1]),
    # agent on (7, 5), flames on (4..6, 5) and (5, 4..6): LEFT walks into (6, 5) and dies in tick 1 (step.cpp:84-98)
    "step_into_flames": ([0, 0, 0, 1, 0, 0], [0, 0, 0, 1, 0, 0]),
    # agent 0 lives and nothing burns within 6 ticks (BOMB: tick 11 is past the horizon); agent 3's rows are below
    "dead_agent": ([0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]),
    # agent on (4, 5); the cross of the bomb on (4, 3), strength 2, is (2..6, 3) and (4, 1..5) and burns in tick 1.  IDLE, BOMB and UP
    # (to (4, 4)) die; DOWN (4, 6) and LEFT (3, 5) are out of it; RIGHT wants (5, 5), which agent 1 coming LEFT from (6, 5) wants
    # too: both stay (HasDPCollision, step.cpp:100-103), and (4, 5) burns ...
    "contested_cell": ([1, 1, 0, 0, 1, 1], [1, 1, 0, 0, 1, 1]),
    "uncontested_cell": ([1, 1, 0, 0, 0, 1], [1, 1, 0, 0, 0, 1]),   # ... with agent 1 idle the step is made
}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_fixture_holds_the_cases_as_they_are_built(oracle, golden):
    cases = MC.all_cases(oracle)
    assert [c.name for c in cases] == list(golden["names"]), "the cases changed: regenerate tests/golden/move_safety.npz"
    assert os.path.getsize(GOLDEN) < 64 * 1024
    for i, c in enumerate(cases):
        assert c.start.tobytes() == golden["start"][i].tobytes(), c.name
        assert bool(golden["has_moves"][i]) == (c.moves is not None) and int(golden["horizon"][i]) == c.horizon, c.name
        assert golden["moves"][i].tolist() == (list(c.moves) if c.moves is not None else [0, 0, 0, 0]), c.name
    assert {1, 4, 12, 32} <= set(golden["horizon"].tolist())
    assert set(HAND) == {c.name for c in MC.hand_made()}


def test_checker_equals_the_reference_on_every_entry(oracle, golden):
    """K x Oracle.step against K x the compiled bboard::Step, the sets on top being the same code; the two invariants of the header
    hold on every row; and the played entries are not quiet"""
    n = len(golden["names"])
    for i in range(n):
        s = golden["start"][i].copy().view(STATE_DTYPE)
        mv = golden["moves"][i:i + 1] if golden["has_moves"][i] else None
        death, escape = move_safety(oracle, s, int(golden["horizon"][i]), mv)
        assert np.array_equal(death[0], golden["death_tick"][i]), golden["names"][i]
        assert np.array_equal(escape[0], golden["escape_tick"][i]), golden["names"][i]
    d, x = golden["death_tick"], golden["escape_tick"]
    assert ((d == -1) == (x == -1)).all()
    assert (x[d == 0] == 0).all() and (x[(d > 0) & (x > 0)] >= d[(d > 0) & (x > 0)]).all()
    played = np.array([nm not in HAND for nm in golden["names"]])
    assert int((d[played] > 0).sum()) >= 100 and int((x[played] > 0).sum()) >= 50 and int(((d[played] > 0) & (x[played] == 0)).sum()) >= 50


def test_hand_written_rows_equal_the_fixture(golden):
    names = list(golden["names"])
    for name, (death, escape) in HAND.items():
        i = names.index(name)
        assert golden["death_tick"][i, 0].tolist() == death, name
        assert golden["escape_tick"][i, 0].tolist() == escape, name
    i = names.index("dead_agent")
    assert golden["death_tick"][i, 3].tolist() == [-1] * 6 and golden["escape_tick"][i, 3].tolist() == [-1] * 6
    # the forecast's own cases say the same of the moves they were recorded with (tests/test_forecast_host.py HAND: agent_tick)
    fc = np.load(os.path.join(ROOT, "tests", "golden", "forecast.npz"))
    fnames = list(fc["names"])
    for name, column in (("move_bomb", FC.B), ("step_out", FC.D), ("stay_in", FC.I), ("step_into_flames", FC.L)):
        mine = "open_corner" if name == "move_bomb" else name
        assert golden["death_tick"][names.index(mine), 0, column] == fc["agent_tick"][fnames.index(name), 0], name


SPEC_PROGRAM = """
#include <stddef.h>
#include "pom_batch.h"
typedef char size_is_stated[sizeof(PomMoveSafetySpec) == POM_MOVE_SAFETY_SPEC_SIZE ? 1 : -1];
typedef char offsets[offsetof(PomMoveSafetySpec, agent_mask) == 8 && offsetof(PomMoveSafetySpec, moves_dev) == 16 &&
                     offsetof(PomMoveSafetySpec, death_tick_dev) == 24 && offsetof(PomMoveSafetySpec, escape_tick_dev) == 32 &&
                     offsetof(PomMoveSafetySpec, reserved2_) == 40 ? 1 : -1];
int use(PomBatch* h)
{
    PomMoveSafetySpec s = {sizeof(PomMoveSafetySpec), 12, 15, 0, 0, 0, 0, 0};
    return pom_batch_move_safety(h, &s);
}
"""


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++17")])
def test_header_compiles_with_the_spec(tmp_path, compiler, std):
    syntax_check(SPEC_PROGRAM, tmp_path, compiler, std)
    assert header_constant("POM_MOVE_SAFETY_SPEC_SIZE") == 48


def test_wrapper_structure_is_the_headers():
    from pomcpp_amd.batch import _MoveSafetySpec
    assert C.sizeof(_MoveSafetySpec) == 48
    assert (_MoveSafetySpec.agent_mask.offset, _MoveSafetySpec.moves_dev.offset, _MoveSafetySpec.death_tick_dev.offset,
            _MoveSafetySpec.escape_tick_dev.offset, _MoveSafetySpec.reserved2_.offset) == (8, 16, 24, 32, 40)


@pytest.fixture(scope="module")
def emul():
    """the kernel's two set functions (pomcpp_amd/csrc/pom_move_safety.h) built for the host"""
    lib = C.CDLL(shared_lib("tests/emul/pom_move_safety_emul.cpp"))
    lib.pom_emul_escape_grow.argtypes = [C.c_void_p] * 3
    lib.pom_emul_escape_grow.restype = None
    lib.pom_emul_free_words.argtypes = [C.c_void_p] * 2
    return lib


def _words(cells):
    """bool [11, 11] (row-major [y][x], cell c = 11 y + x) -> the 121-bit set as four little-endian words"""
    bits = np.zeros(128, dtype=np.uint8)
    bits[:121] = cells.reshape(121)
    return np.packbits(bits, bitorder="little").view("<u4").copy()


def test_host_compiled_growth_step_equals_the_boolean_one(emul):
    """random sets and Free masks of every density, and every single cell by itself on a full Free mask — the edge columns and rows,
    where a shift must not wrap a row's end into the next row's start, included"""
    rng = np.random.default_rng(5)
    trials = [(rng.random((11, 11)) < p, rng.random((11, 11)) < q) for p in (0.02, 0.1, 0.5, 0.9) for q in (0.3, 0.7, 1.0) for _ in range(40)]
    full = np.ones((11, 11), dtype=bool)
    for c in range(121):
        one = np.zeros((11, 11), dtype=bool)
        one[c // 11, c % 11] = True
        trials.append((one, full))
        trials.append((~one, full))
    for x in (0, 10):   # a whole edge column, a whole edge row
        col, row = np.zeros((11, 11), dtype=bool), np.zeros((11, 11), dtype=bool)
        col[:, x], row[x, :] = True, True
        trials += [(col, full), (row, full)]
    for reach, free in trials:
        r, f, out = _words(reach), _words(free), np.zeros(4, dtype=np.uint32)
        emul.pom_emul_escape_grow(r.ctypes.data, f.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, _words(grow(reach, free))), np.argwhere(reach).tolist()


def test_host_compiled_free_word_equals_the_boards_free_cells(emul, oracle):
    """Free through pack -> cell codes -> the kernel's classification, against the State's board values: played boards of both kinds
    (passages, power-ups, wood, bombs, flames with and without a power-up under them, agents)"""
    seen = set()
    for kind, ticks in (("ffa", 57), ("stress", 23)):
        states = FC.played_states(oracle, kind, 48, ticks)
        for e in range(states.size):
            out = np.zeros(4, dtype=np.uint32)
            assert emul.pom_emul_free_words(states[e:e + 1].ctypes.data, out.ctypes.data) == 0
            free = free_cells(states["board"][e])
            assert np.array_equal(out, _words(free)), (kind, e)
            seen |= set(np.unique(states["board"][e][free]).tolist())
    assert seen == {0, 6, 7, 8}   # passage and all three power-ups were among the free cells
    s = pa.new_states(1)          # an empty board: all 121 cells, and nothing past them
    out = np.zeros(4, dtype=np.uint32)
    assert emul.pom_emul_free_words(s.ctypes.data, out.ctypes.data) == 0 and out.tolist() == [0xFFFFFFFF] * 3 + [0x01FFFFFF]
